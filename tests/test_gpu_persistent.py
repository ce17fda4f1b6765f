"""The persistent Hiera kernels (csrc/hiera.hip) beyond one pass per workgroup.

Each of them is launched with one workgroup per CU and walks several work units, carrying state from one to the next: attn8 its
LDS-resident weights, the streamed kernels (attn4, attnp, attnq, mlp112, mlp224) a four-slot weight ring whose phase at the start of a
group depends on the groups the workgroup ran before (tests/hieraref.py: "pass", "start slot").  The shapes of
tests/test_gpu_kernels.py fit in one pass; here the unit counts scale with the device's CU count so that every start slot is reached
and a PARTIAL last group lies on pass 2 or later:

    attn8 (LayerNorm inside | h given)   2 * 4 * CU + 6 windows          attnq   (4 CU + 2) * 16 + 5 windows   slots 0 3 2 1 0
    attn4                                (2 CU + 2) * 16 + 5 windows     mlp112  (4 CU + 2) * 384 + 100 rows   slots 0 3 2 1 0
    attnp                                (2 CU + 2) * 8 + 3 windows      mlp224  (2 CU + 2) * 256 + 100 rows
                                         (slots 0 2 0)

rounded up to whole small images (hieraref.GEOM: 4 windows each — 6 for attn8, whose pass is 4 windows) so that the image index,
both window coordinates and chunking by whole images vary.  Every case asserts
  a. coverage, before anything is launched: by hieraref.walk the sample holds a whole group of every (pass, start slot), the first
     group, the last full group and the partial last group, which lies on pass >= 2;
  b. ratio(kernel, float64 reference) <= C_FUSED on the sample, finite everywhere; the unfused launches of the same library are run
     beside it — C_FUSED is twice THEIR largest ratio, never the fused kernels';
  c. three unequal chunks of whole images (each a single pass) and one image alone give the bits of the whole launch;
  d. for the in-place kernels x is a column view inside a sentinel-filled buffer and x16 / h_next the head of longer buffers: every
     cell outside keeps the sentinel, also on the late pass whose dead lanes compute on window 0 and store nothing."""
import pytest
import torch

import hieraref as R

pytestmark = pytest.mark.gpu

CASES = [("attn8", "ln"), ("attn8", "h"), ("attn4", "h"), ("attnp", "h"), ("attnq", "h"), ("mlp112", "h"), ("mlp224", "h")]
COL0, GAP, EXTRA = 8, 16, 5  # x = buf[:rows, 8:8 + D] of a buffer with row stride D + 24 and 5 more rows


def target_units(kernel, cu):
    g = R.GEOM[kernel]["per_group"]
    return {"attn8": 2 * 4 * cu + 6, "attn4": (2 * cu + 2) * g + 5, "attnp": (2 * cu + 2) * g + 3, "attnq": (4 * cu + 2) * g + 5,
            "mlp112": (4 * cu + 2) * g + 100, "mlp224": (2 * cu + 2) * g + 100}[kernel]


class Plan:
    """Sizes, walk and sample of one case on a device of `cu` CUs."""

    def __init__(self, kernel, cu):
        g = R.GEOM[kernel]
        self.kernel, self.cu, self.pg = kernel, cu, g["per_group"]
        self.mlp = kernel.startswith("mlp")
        if self.mlp:
            self.per_img = 64            # rows of the "images" the chunks are cut along
            self.units = target_units(kernel, cu)
            self.rows = self.units
        else:
            self.Gh, self.Gw = g["img"]
            self.ws = g["ws"]
            self.per_img = (self.Gh // self.ws) * (self.Gw // self.ws)
            self.units = R.round_up_partial(target_units(kernel, cu), self.per_img, self.pg)
            self.n_img = self.units // self.per_img
            self.rows = self.n_img * self.Gh * self.Gw
        self.ng = R.n_groups(kernel, self.units)
        assert self.units % self.pg != 0, "the last group must be partial"
        if kernel == "attn8":  # the walk's unit is a window: a group is the four windows of one workgroup pass
            w = R.walk(kernel, self.units, cu)
            self.walk = [w[4 * i] for i in range(self.ng)]
            assert all(w[j] == self.walk[j // 4] for j in range(self.units))
        else:
            self.walk = R.walk(kernel, self.ng, cu)
        # the sample: first group, last full group, partial last group, and the first and a middle group of every pass
        phases = sorted({(p, s) for _, p, s in self.walk})
        pick = {0, self.ng - 2, self.ng - 1}
        for ph in phases:
            of = [i for i, u in enumerate(self.walk) if u[1:] == ph]
            pick |= {of[0], of[len(of) // 2]}
        self.sample = sorted(pick)
        self.phases = phases

    def group_units(self, grp):
        return range(grp * self.pg, min((grp + 1) * self.pg, self.units))

    def check_coverage(self, slots):
        full = [i for i in self.sample if len(self.group_units(i)) == self.pg]
        assert {self.walk[i][1:] for i in full} == set(self.phases), "a (pass, start slot) without a whole sampled group"
        assert [s for _, s in self.phases] == slots, f"start slots by pass {self.phases}"
        assert 0 in self.sample and self.ng - 2 in full and self.ng - 1 in self.sample
        assert len(self.group_units(self.ng - 1)) < self.pg and self.walk[self.ng - 1][1] >= 2, "partial last group on pass >= 2"
        assert max(p for _, p, _ in self.walk) == len(slots) - 1

    def in_rows(self, units):
        """Input token rows [len(units), T] of windows (the MLP: the rows themselves)."""
        if self.mlp:
            return torch.tensor(list(units))
        return R.window_rows(list(units), self.Gh, self.Gw, self.ws)

    def out_rows(self, units):
        if R.GEOM[self.kernel].get("pool"):
            return R.window_rows(list(units), self.Gh // 2, self.Gw // 2, self.ws // 2)
        return self.in_rows(units)

    def chunks(self):
        """Three unequal ranges of whole images (start, mid, end of the launch) and one image alone -> [(unit0, unit1)]."""
        n = self.units // self.per_img  # whole images (the MLP's trailing rows ride with the last chunk)
        sizes = (3, 5, 9) if not self.mlp else (13, 10, 21)
        starts = (0, n // 2, n - sizes[2])
        lone = (self.ng - 2) * self.pg // self.per_img  # the image that holds the first unit of the last full group
        out = [(s * self.per_img, (s + k) * self.per_img) for s, k in zip(starts, sizes)] + [(lone * self.per_img, (lone + 1) * self.per_img)]
        out[2] = (out[2][0], self.units)
        for u0, u1 in out:
            groups = -(-(u1 - u0) // (4 if self.kernel == "attn8" else self.pg))
            assert 0 <= u0 < u1 <= self.units and groups <= self.cu, "a chunk must be a single pass"
        return out


EXPECTED_SLOTS = {"attn8": [0, 0, 0], "attn4": [0, 0, 0], "attnp": [0, 2, 0], "attnq": [0, 3, 2, 1, 0], "mlp112": [0, 3, 2, 1, 0],
                  "mlp224": [0, 0, 0]}


# ------------------------------------------------------------------------------------------------ launches
class Runner:
    """The fused kernel and the unfused launches it replaces, on rows [r0, r1) of the case's inputs."""

    def __init__(self, kernel, form, pl, cuda):
        from lmx import sam

        self.kernel, self.form, self.pl, self.dev = kernel, form, pl, cuda
        self.g = R.GEOM[kernel]
        gen = torch.Generator(device=cuda).manual_seed(1000 + 10 * CASES.index((kernel, form)))
        self.p = R.make_params(kernel, gen, cuda)
        self.x0, self.h = R.make_acts(kernel, pl.rows, gen, cuda)
        n = {k: v.cpu().numpy() for k, v in self.p.items()}
        heads = self.g.get("heads")
        if pl.mlp:
            packed = sam.pack_ln_mlp(n["w1"], n["b1"], n["w2"], n["b2"], n["g2"], n["e2"], n["gn"], n["en"])
        elif self.g["pool"]:
            packed = sam.pack_hiera_attn_pool(n["wsc"], n["bsc"], n["wqkv"], n["bqkv"], n["wo"], n["bo"], heads)
        elif kernel == "attn8":
            packed = sam.pack_hiera_attn(n["wqkv"], n["bqkv"], n["wo"], n["bo"], heads, ln_inside=form == "ln")
        else:
            packed = sam.pack_hiera_attn4(n["wqkv"], n["bqkv"], n["wo"], n["bo"], heads)
        if not pl.mlp and kernel != "attn8":
            assert packed[0].shape[0] == R.images_per_group(kernel)
        self.packed = tuple(torch.from_numpy(a).to(cuda) for a in packed)
        self.w16 = {k: v.half() for k, v in self.p.items() if k.startswith("w")}

    def rows_of(self, u0, u1):
        """Token rows [r0, r1) of units [u0, u1) that are whole images (the MLP: rows)."""
        if self.pl.mlp:
            return u0, u1
        per = self.pl.Gh * self.pl.Gw
        assert u0 % self.pl.per_img == 0 and u1 % self.pl.per_img == 0
        return u0 // self.pl.per_img * per, u1 // self.pl.per_img * per

    def fused(self, x, r0, r1, x16=None, h_next=None):
        """x: the f32 rows to update in place (any row stride), None for the pooled kernels -> the result rows."""
        from lmx import kernels as K

        pl, p = self.pl, self.p
        if pl.mlp:
            return K.ln_mlp_img(x, self.packed, R.EPS, x16=x16, h_next=h_next)
        n_img = (r1 - r0) // (pl.Gh * pl.Gw)
        h = self.h[r0:r1]
        heads = self.g["heads"]
        if self.g["pool"]:
            return K.hiera_attn_pool(h, self.packed, n_img, pl.Gh, pl.Gw, heads, self.g["D"])
        if self.kernel == "attn4":
            return K.hiera_attn4(h, x, self.packed, n_img, pl.Gh, pl.Gw, heads)
        if self.form == "ln":
            return K.hiera_attn8(x, self.packed, n_img, pl.Gh, pl.Gw, heads, ln=(p["gam"], p["bet"], R.EPS))
        return K.hiera_attn8(x, self.packed, n_img, pl.Gh, pl.Gw, heads, h=h)

    def unfused(self):
        """The launches the kernel replaces (tests/test_gpu_kernels.py runs the same chains), on the whole input -> result rows
        (the MLP: (x, h_next))."""
        from lmx import kernels as K

        pl, p, w16, g = self.pl, self.p, self.w16, self.g
        if pl.mlp:
            xu = self.x0.clone()
            hn = torch.empty((pl.rows, g["D"]), dtype=torch.float16, device=self.dev)
            K.ln_mlp(xu, p["g2"], p["e2"], w16["w1"], p["b1"], w16["w2"], p["b2"], R.EPS, next_ln=(p["gn"], p["en"], hn))
            return xu, hn
        D, heads, ws, n, Gh, Gw = g["D"], g["heads"], pl.ws, pl.n_img, pl.Gh, pl.Gw
        hd = D // heads
        h = K.layernorm(self.x0, p["gam"], p["bet"], R.EPS) if self.form == "ln" else self.h
        q3 = K.gemm(h, w16["wqkv"], bias=p["bqkv"])
        pads = dict(pad_k=q3[0, D:2 * D].contiguous(), pad_v=q3[0, 2 * D:].contiguous())
        if not g["pool"]:
            a = torch.empty((pl.rows, D), dtype=torch.float16, device=self.dev)
            K.attention(q3[:, :D], q3[:, D:2 * D], q3[:, 2 * D:], a, pl.units, heads, ws * ws, ws * ws, hd, hd ** -0.5,
                        window=dict(Gh=Gh, Gw=Gw, ws=ws, q_stride=1), **pads)
            xu = self.x0.clone()
            K.gemm(a, w16["wo"], bias=p["bo"], res=xu, out=xu)
            return xu
        scu = K.gemm(h, w16["wsc"], bias=p["bsc"], out_dtype=torch.float32)
        pooled = torch.empty((n, Gh // 2, Gw // 2, D), dtype=torch.float32, device=self.dev)
        K.maxpool2(scu.view(n, Gh, Gw, D), pooled)
        del scu
        qp = torch.empty((n, Gh // 2, Gw // 2, D), dtype=torch.float16, device=self.dev)
        K.maxpool2(q3.view(n, Gh, Gw, 3 * D)[..., :D], qp)
        wq = ws // 2
        a = torch.empty((pl.rows // 4, D), dtype=torch.float16, device=self.dev)
        K.attention(qp.view(-1, D), q3[:, D:2 * D], q3[:, 2 * D:], a, pl.units, heads, wq * wq, ws * ws, hd, hd ** -0.5,
                    window=dict(Gh=Gh, Gw=Gw, ws=ws, q_stride=2), **pads)
        xu = torch.empty((pl.rows // 4, D), dtype=torch.float32, device=self.dev)
        K.gemm(a, w16["wo"], bias=p["bo"], res=pooled.view(-1, D), out=xu)
        return xu


def _guarded(rows, D, dtype, cuda, col0=COL0, gap=GAP):
    """(buffer, view): view = buffer[:rows, col0:col0 + D] of a sentinel-filled [rows + EXTRA, col0 + D + gap] buffer."""
    buf = torch.full((rows + EXTRA, col0 + D + gap), R.SENT, dtype=dtype, device=cuda)
    return buf, buf[:rows, col0:col0 + D]


def _sentinels_intact(buf, rows, D, col0=COL0):
    return bool((buf[:, :col0] == R.SENT).all()) and bool((buf[:, col0 + D:] == R.SENT).all()) and bool((buf[rows:] == R.SENT).all())


@pytest.mark.parametrize("kernel,form", CASES, ids=[f"{k}-{f}" for k, f in CASES])
def test_late_passes(cuda, kernel, form):
    cu = torch.cuda.get_device_properties(cuda).multi_processor_count
    pl = Plan(kernel, cu)
    pl.check_coverage(EXPECTED_SLOTS[kernel])                                                   # a. before any launch
    chunks = pl.chunks()
    run = Runner(kernel, form, pl, cuda)
    D, pool, tag = run.g["D"], run.g.get("pool", False), f"persistent {kernel} {form}"
    print(f"{tag}: {cu} CUs, {pl.units} units in {pl.ng} groups of {pl.pg}, {R.images_per_group(kernel)} images per group, "
          f"last group {len(pl.group_units(pl.ng - 1))} units on pass {pl.walk[-1][1]}, sample of {len(pl.sample)} groups")

    # ---- the whole launch, guarded (d)
    x16 = hn = xbuf = None
    if pool:
        whole = run.fused(None, 0, pl.rows)
    else:
        xbuf, whole = _guarded(pl.rows, D, torch.float32, cuda)
        whole.copy_(run.x0)
        if pl.mlp:  # x16 / h_next: the first rows of longer contiguous buffers
            b16, bhn = (torch.full((pl.rows + EXTRA, D), R.SENT, dtype=torch.float16, device=cuda) for _ in range(2))
            x16, hn = b16[:pl.rows], bhn[:pl.rows]
        run.fused(whole, 0, pl.rows, x16=x16, h_next=hn)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(whole).all()), "non-finite result"
    if xbuf is not None:
        assert _sentinels_intact(xbuf, pl.rows, D), "cells outside x were written"
    if pl.mlp:
        assert bool((b16[pl.rows:] == R.SENT).all()) and bool((bhn[pl.rows:] == R.SENT).all()), "rows past x16 / h_next were written"
        assert bool(torch.isfinite(hn).all()) and torch.equal(x16, whole.half())
    unf = run.unfused()

    # ---- b. float64 on the sample, per sampled group
    pc = R.f64(run.p)
    worst, worst_u, lines = (0.0, None), 0.0, []
    for grp in pl.sample:
        units = pl.group_units(grp)
        rin, rout = pl.in_rows(units).to(cuda), pl.out_rows(units).to(cuda)
        xs = run.x0[rin].cpu() if run.x0 is not None else None
        hs = run.h[rin].cpu() if run.h is not None and form == "h" and not pl.mlp else None
        ref = R.reference(kernel, xs, hs, pc, form=form)
        if pl.mlp:
            r = max(R.ratio(whole[rout].cpu(), ref[:, :D]), R.ratio(hn[rout].cpu(), ref[:, D:]))
            ru = max(R.ratio(unf[0][rout].cpu(), ref[:, :D]), R.ratio(unf[1][rout].cpu(), ref[:, D:]))
        else:
            r, ru = R.ratio(whole[rout].cpu(), ref), R.ratio(unf[rout].cpu(), ref)
        wg, p, s = pl.walk[grp]
        lines.append(f"{tag}: group {grp} ({len(units)} units) workgroup {wg} pass {p} slot {s}: fused {R.lg(r)} unfused {R.lg(ru)}")
        worst, worst_u = max(worst, (r, (p, s))), max(worst_u, ru)
    print("\n".join(lines))
    print(f"{tag}: max ratio {R.lg(worst[0])} at (pass, slot) {worst[1]}, unfused launches {R.lg(worst_u)} (bound {R.lg(R.C_FUSED)})")
    del unf
    assert worst[0] <= R.C_FUSED, f"{tag}: {R.lg(worst[0])} > {R.lg(R.C_FUSED)} at (pass, slot) {worst[1]}"
    assert worst_u <= R.C_FUSED / 2 * 1.01, f"{tag}: the unfused launches reach {R.lg(worst_u)}: C_FUSED is no longer twice their ratio"

    # ---- c. placement does not change the bits
    for u0, u1 in chunks:
        r0, r1 = run.rows_of(u0, u1)
        o0, o1 = (r0 // 4, r1 // 4) if pool else (r0, r1)
        if pool:
            got = run.fused(None, r0, r1)
        elif pl.mlp:
            c16, chn = (torch.empty((r1 - r0, D), dtype=torch.float16, device=cuda) for _ in range(2))
            got = run.fused(run.x0[r0:r1].clone(), r0, r1, x16=c16, h_next=chn)
            assert torch.equal(c16, x16[o0:o1]) and torch.equal(chn, hn[o0:o1]), f"{tag}: x16 / h_next of units {u0}..{u1} alone differ"
        else:
            got = run.fused(run.x0[r0:r1].clone(), r0, r1)
        if not torch.equal(got, whole[o0:o1]):
            bad = (got != whole[o0:o1]).any(1).nonzero().flatten()
            raise AssertionError(f"{tag}: units {u0}..{u1} alone differ from the whole launch in {len(bad)} rows, first {bad[:8].tolist()}")
    print(f"{tag}: chunks {chunks} bitwise equal to the whole launch")
    del run, whole, xbuf, x16, hn
    torch.cuda.empty_cache()
