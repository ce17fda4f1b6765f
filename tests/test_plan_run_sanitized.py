"""csrc/plan_run.h hands every native model its device buffers: offsets inside an allocation that a counting walk sized, which the
launching walk then writes behind.  Its arithmetic therefore runs once under AddressSanitizer and UndefinedBehaviorSanitizer: as a
stand-alone program (tests/plan_run_check_main.cpp), on the CPU, in a child process; nothing is loaded into this interpreter.  The
program walks a toy plan twice — counting, then launching into heap blocks of exactly the counted sizes, filling every buffer — and
checks the offsets, the peaks across a rewind, the largest-request region, the alignment and every refusal; it must exit 0 with an
empty stderr (no sanitizer report)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "plan_run_check_main.cpp")
FLAGS = ["-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_plan_run_is_clean_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "plan_run_check_main"
    subprocess.run(["g++", *FLAGS, SOURCE, "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    assert run.stderr == "", run.stderr[-2000:]
    assert run.stdout == "ok\n"
