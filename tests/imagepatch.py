"""Corrupting a weight image (csrc/image.h) for the tests of its readers: find a tensor's directory entry, overwrite one field."""
import struct

from lmx import native


def entry_offset(raw, name):
    """the file offset of the 88-byte directory entry of tensor `name`"""
    dir_off, n = struct.unpack_from("<Q", raw, 24)[0], struct.unpack_from("<I", raw, 20)[0]
    for i in range(n):
        at = dir_off + i * native.ENTRY_BYTES
        if raw[at:at + native.NAME_BYTES].rstrip(b"\0") == name.encode():
            return at
    raise KeyError(name)


def patch(raw, at, fmt, value):
    """`raw` with `value` packed as `fmt` at offset `at`"""
    b = bytearray(raw)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)
