"""The sparse loss kernels (csrc/losses.hip) PER ELEMENT against the fp64 restatements of tests/loss_ref64.py: |got - ref64| <= bound(element), the
bound derived there from the kernel's operations, never measured; bound 0 (equality) for the structural zeros; torch.equal for the one kernel that is
a single fp32 product.  A failure reports the worst err / bound and its index.  tests/test_loss_ref_host.py shows on the CPU that wrong restatements
fail these bounds at these inputs.

Every entry point is called through lib() with each output inside a NaN-filled buffer: every element must be written, the guard regions either side
must keep their bits.  Whatever lies at or beyond counts is NaN on the way in — rows of u, entries of depth, d1, d2 and pts3d, rows and columns of
sim: rows at or beyond counts never influence an output (include/gd_hip.h), and the matching output rows come back as zeros.

Kernel, arm -> case:
  pair_rank_tile_kernel        (pair_rank_wave 0)  test_pair_rank[0-*]: ragged (18: valid pairs and padding slots in one wave; 17: row 16 alone; 1, 0),
                                                   seams (Nmax 70: 5 x 3 tiles, counts None and [70, 65, 64, 33, 32, 31]), exact mask; both heads
  pair_rank_kernel             (pair_rank_wave 1)  test_pair_rank[1-*]     the same cases
  pair_rank8_kernel<16>, <8>   (pair_rank_wave 2, 3)  test_pair_rank[2-*], [3-*]
  pair_rank_finalize_kernel    every test_pair_rank: gscale None | per set with 0 and a negative one; head_grad accumulated into, head_grad_sets[:, 513:] = 0
  depth_l1_kernel, row_sum_cols_kernel   test_depth_l1: Nmax 21 = a 16-keypoint block and 5, counts [21, 16, 5, 0]; per-set rows given | in the workspace
  depth_head_fwd_kernel, depth_head_bwd_kernel   test_depth_head[M]: 32-row blocks, M in {1, 31, 32, 33, 70}
  smooth_ap_kernel, row_sum_kernel       test_smooth_ap[shape-variant]: Nmax 264 past the 256-thread stride, counts [264, 257, 256, 1]; Nmax 24, counts None
  smooth_ap_me_kernel, smooth_ap_me_finalize_kernel   test_smooth_ap_me[shape]; Nmax 4097 refused before any launch: test_smooth_ap_me_refuses_4097
  depth_bwd_combine_kernel     test_depth_bwd_combine[pair_major | view_major]
  scale_and_transpose_kernel   test_scale_and_transpose
  loss_combine_fwd_kernel, loss_combine_bwd_kernel    tests/test_gpu_ops.py::test_loss_combine_matches_the_weighted_sum_and_mean (held to the torch expression there)"""
import contextlib
import functools

import pytest
import torch

import loss_ref64 as L

pytestmark = pytest.mark.gpu

F32 = torch.float32
GUARD = 64                    # elements either side of an output
NAN = float("nan")
PREFILL = 0.625               # head_grad is accumulated into: it arrives holding this


def _check(got, ref, bound, what):
    """Every element: |got - ref| <= bound (bound 0: equality; a NaN anywhere fails)."""
    err = (got.detach().double().cpu() - ref.double()).abs()
    bound = bound.double().expand_as(err)
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    if ratio.numel() == 0:
        return
    worst, i = float(ratio.max()), int(ratio.argmax())
    idx = tuple(int(t) for t in torch.unravel_index(torch.tensor(i), ratio.shape))
    print(f"{what}: worst err / bound = {worst:.4f} at {idx}")
    assert worst <= 1.0, (f"{what}: worst err / bound = {worst:.3f} at {idx}: got {float(got.double().reshape(-1)[i])!r}, "
                          f"ref {float(ref.double().reshape(-1)[i])!r}, bound {float(bound.reshape(-1)[i]):.3e}")


def _checkv(got, ref, what):
    _check(got, ref.v, L.bound(ref), what)


class _Guarded:
    """An fp32 output of `shape` inside a NaN-filled buffer (fill: what an accumulated-into output holds on the way in)."""

    def __init__(self, shape, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD,), NAN, dtype=F32, device="cuda")
        self.lo, self.n = GUARD, n
        self.out = self.buf[self.lo:self.lo + n].view(shape)
        if fill is not None:
            self.out.fill_(fill)
        self.before = self.buf.view(torch.int32).clone()

    def done(self, what, all_written=True):
        torch.cuda.synchronize()
        b = self.buf.view(torch.int32)
        assert torch.equal(b[:self.lo], self.before[:self.lo]) and torch.equal(b[self.lo + self.n:], self.before[self.lo + self.n:]), \
            f"{what}: wrote outside its output"
        if all_written:
            assert not torch.isnan(self.out).any(), f"{what}: left part of its output unwritten, or wrote NaN there"
        return self.out


def _pad_nan(t, counts, dims=(1,)):
    """A CUDA copy of t [sets, ...] with everything at or beyond counts[set] along `dims` NaN."""
    t = t.clone()
    if counts is not None:
        for s, n in enumerate(counts.tolist()):
            for d in dims:
                t[s].narrow(d - 1, n, t.shape[d] - n).fill_(NAN)
    return t.cuda()


def _hp(hp):
    return [hp[k].cuda().contiguous() for k in ("b1", "ln_w", "ln_b", "w2", "b2")]


@contextlib.contextmanager
def _pair_rank_wave(form):
    from gd_amd._lib import check, lib
    prev = lib().gd_debug_get(b"pair_rank_wave")
    check(lib().gd_debug_set(b"pair_rank_wave", form), "gd_debug_set")
    try:
        yield
    finally:
        check(lib().gd_debug_set(b"pair_rank_wave", prev), "gd_debug_set")


def _head_grad(got, ref_sum, n_adds, what):
    """head_grad arrived holding PREFILL: it leaves as PREFILL + the sum, gained in n_adds atomic additions ([513:] untouched)."""
    _check(got, PREFILL + ref_sum.v, L.head_grad_bound(ref_sum, PREFILL, n_adds), what)
    assert torch.equal(got[513:].cpu(), torch.full((3,), PREFILL)), f"{what}: head_grad[513:] touched"


# ------------------------------------------------------------------------------------------------ gd_pair_rank, four forms
@functools.lru_cache(maxsize=None)
def _rank_ref(name, head):
    inp = L.rank_inputs(name, head)
    return inp, L.rank_case(inp)


@pytest.mark.parametrize("head", L.HEAD_NAMES)
@pytest.mark.parametrize("name", list(L.RANK_CASES))
@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_pair_rank(form, name, head):
    """Loss, du, the per-set and the accumulated head gradients and the exact ordered-pair count of every form, with NaN in every padding row."""
    from gd_amd._lib import check, lib, ptr, stream
    inp, ref = _rank_ref(name, head)
    S, Nmax = inp.S, inp.Nmax
    u, depth = _pad_nan(inp.u, inp.counts), _pad_nan(inp.depth, inp.counts)
    counts = None if inp.counts is None else inp.counts.cuda()
    gscale = None if inp.gscale is None else inp.gscale.cuda()
    hp = _hp(inp.hp)
    loss, du, hgs, hg = _Guarded((S,)), _Guarded((S, Nmax, 128)), _Guarded((S, L.HG)), _Guarded((L.HG,), PREFILL)
    nws = lib().gd_pair_rank_workspace_bytes(S)
    assert nws == S * (L.HG + 2) * 4
    ws = _Guarded((nws // 4,))
    with _pair_rank_wave(form):
        assert lib().gd_debug_get(b"pair_rank_wave") == form
        check(lib().gd_pair_rank(ptr(u), ptr(depth), ptr(counts), ptr(gscale), S, Nmax, float(inp.thr), *[ptr(t) for t in hp], ptr(loss.out),
                                 ptr(du.out), ptr(hg.out), ptr(hgs.out), ptr(ws.out), stream()), "gd_pair_rank")
        torch.cuda.synchronize()
    what = f"gd_pair_rank form {form} {name} {head}"
    cnt = ws.done(what, all_written=False)[S * (L.HG + 1):].view(torch.int32).cpu().tolist()          # workspace: hg [S, 516] | loss_sum [S] | pair_cnt [S] (int)
    assert cnt == ref["cnt"], f"{what}: ordered-pair counts {cnt}, expected {ref['cnt']}"
    _checkv(loss.done(what), ref["loss"], what + " loss")
    _checkv(du.done(what), ref["du"], what + " du")
    _checkv(hgs.done(what), ref["hg_sets"], what + " head_grad_sets")
    _head_grad(hg.done(what), ref["hg_sum"], S, what + " head_grad")


def test_pair_rank_optional_outputs():
    """head_grad and head_grad_sets are each nullable: the other outputs do not change."""
    from gd_amd._lib import check, lib, ptr, stream
    inp, ref = _rank_ref("ragged_1", "active")
    u, depth, counts, gscale, hp = _pad_nan(inp.u, inp.counts), _pad_nan(inp.depth, inp.counts), inp.counts.cuda(), inp.gscale.cuda(), _hp(inp.hp)
    for with_sum in (False, True):
        loss, du = _Guarded((inp.S,)), _Guarded((inp.S, inp.Nmax, 128))
        hg, hgs = (_Guarded((L.HG,), PREFILL), None) if with_sum else (None, _Guarded((inp.S, L.HG)))
        ws = _Guarded((inp.S * (L.HG + 2),))
        check(lib().gd_pair_rank(ptr(u), ptr(depth), ptr(counts), ptr(gscale), inp.S, inp.Nmax, float(inp.thr), *[ptr(t) for t in hp], ptr(loss.out),
                                 ptr(du.out), ptr(hg.out) if hg else None, ptr(hgs.out) if hgs else None, ptr(ws.out), stream()), "gd_pair_rank")
        what = f"gd_pair_rank head_grad {'only' if with_sum else 'absent'}"
        _checkv(loss.done(what), ref["loss"], what + " loss")
        _checkv(du.done(what), ref["du"], what + " du")
        if with_sum:
            _head_grad(hg.done(what), ref["hg_sum"], inp.S, what)
        else:
            _checkv(hgs.done(what), ref["hg_sets"], what + " head_grad_sets")


# ------------------------------------------------------------------------------------------------ gd_depth_l1, gd_depth_head_*
@pytest.mark.parametrize("arm", ["sets", "workspace"])
@pytest.mark.parametrize("fscale", [1.0, 0.05])
def test_depth_l1(fscale, arm):
    """counts [21, 16, 5, 0] of Nmax 21: a full 16-keypoint block and a partial one, a set that ends at the block seam, an empty set.  arm: the
    per-set head gradients go to head_grad_sets, or to the workspace when the caller does not want them (gscale then NULL)."""
    from gd_amd._lib import check, lib, ptr, stream
    inp = L.l1_inputs(fscale, with_gscale=arm == "sets")
    ref = L.l1_case(inp)
    P, Nmax = 4, inp.Nmax
    u = _pad_nan(inp.u, inp.counts, dims=(2,))
    d1, d2, counts = _pad_nan(inp.d1, inp.counts), _pad_nan(inp.d2, inp.counts), inp.counts.cuda()
    gscale = None if inp.gscale is None else inp.gscale.cuda()
    hp = _hp(inp.hp)
    loss, du, hg, rows = _Guarded((P,)), _Guarded((P, 2, Nmax, 128)), _Guarded((L.HG,), PREFILL), _Guarded((P, L.HG))
    sets, ws = (rows.out, None) if arm == "sets" else (None, rows.out)
    check(lib().gd_depth_l1(ptr(u), ptr(d1), ptr(d2), ptr(counts), ptr(gscale), P, Nmax, *[ptr(t) for t in hp], ptr(loss.out), ptr(du.out), ptr(hg.out),
                            ptr(sets), ptr(ws), stream()), "gd_depth_l1")
    what = f"gd_depth_l1 scale {fscale} {arm}"
    _checkv(loss.done(what), ref["loss"], what + " loss")
    _checkv(du.done(what), ref["du"], what + " du")
    _checkv(rows.done(what), ref["hg_sets"], what + " per-set head gradients")
    _check(hg.done(what), PREFILL + ref["hg_sum"].v, L.head_grad_bound(ref["hg_sum"], PREFILL, 1), what + " head_grad")      # one += of the column sums


@pytest.mark.parametrize("M", L.HEAD_M)
@pytest.mark.parametrize("fscale", [1.0, 0.05])
def test_depth_head(fscale, M):
    from gd_amd._lib import check, lib, ptr, stream
    rows, dout, hpr = L.head_inputs(M, fscale)
    s, dz, hgr = L.head_rows(rows, hpr, dout)
    u, dy, hp = rows.cuda(), dout.cuda(), _hp(hpr)
    out, du, hg = _Guarded((M,)), _Guarded((M, 128)), _Guarded((L.HG,), PREFILL)
    check(lib().gd_depth_head_fwd(ptr(u), M, *[ptr(t) for t in hp], ptr(out.out), stream()), "gd_depth_head_fwd")
    check(lib().gd_depth_head_bwd(ptr(u), ptr(dy), M, *[ptr(t) for t in hp], ptr(du.out), ptr(hg.out), stream()), "gd_depth_head_bwd")
    what = f"gd_depth_head M {M} scale {fscale}"
    _checkv(out.done(what), s, what + " fwd")
    _checkv(du.done(what), dz, what + " du")
    _head_grad(hg.done(what), hgr, (M + 31) // 32, what + " head_grad")          # one set of atomics per 32-row block


# ------------------------------------------------------------------------------------------------ smooth-AP
def _ap_args(inp):
    dims = (1, 2)
    return (_pad_nan(inp.sim, inp.counts, dims), _pad_nan(inp.p1, inp.counts), _pad_nan(inp.p2, inp.counts),
            None if inp.counts is None else inp.counts.cuda())


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("shape", list(L.AP_SHAPES))
def test_smooth_ap(shape, variant):
    """loss, dsim and row_ws as functions of the GIVEN sim: active sigmoids, both saturated sides (derivative exactly 0), exponents either side of the
    clamp; coincident off-diagonal points, a diagonal pair beyond the threshold; rows and columns at or beyond counts NaN in, zero out."""
    from gd_amd._lib import check, lib, ptr, stream
    inp = L.ap_inputs(shape)
    ref = L.ap_case(inp, variant)
    P, N = inp.sim.shape[:2]
    sim, p1, p2, counts = _ap_args(inp)
    loss, dsim, rows = _Guarded((P,)), _Guarded((P, N, N)), _Guarded((P, N))
    check(lib().gd_smooth_ap(ptr(sim), ptr(p1), ptr(p2), ptr(counts), P, N, variant, float(inp.thr_neg), float(inp.temp), ptr(loss.out), ptr(dsim.out),
                             ptr(rows.out), stream()), "gd_smooth_ap")
    what = f"gd_smooth_ap {shape} variant {variant}"
    _checkv(loss.done(what), ref["loss"], what + " loss")
    _checkv(rows.done(what), ref["rows"], what + " row_ws")
    _checkv(dsim.done(what), ref["dsim"], what + " dsim")


@pytest.mark.parametrize("shape", list(L.AP_SHAPES))
def test_smooth_ap_me(shape):
    """Rows with 0, 1 and 3 positives; one pair with no positive at all: loss 0 and an all-zero dsim (bound 0)."""
    from gd_amd._lib import check, lib, ptr, stream
    inp = L.ap_inputs(shape, me=True)
    ref = L.me_case(inp)
    P, N = inp.sim.shape[:2]
    sim, p1, p2, counts = _ap_args(inp)
    loss, dsim, rows = _Guarded((P,)), _Guarded((P, N, N)), _Guarded((P, N, 2))
    check(lib().gd_smooth_ap_me(ptr(sim), ptr(p1), ptr(p2), ptr(counts), P, N, float(inp.thr_pos), float(inp.thr_neg), float(inp.temp), ptr(loss.out),
                                ptr(dsim.out), ptr(rows.out), stream()), "gd_smooth_ap_me")
    what = f"gd_smooth_ap_me {shape}"
    _checkv(loss.done(what), ref["loss"], what + " loss")
    _checkv(rows.done(what), ref["rows"], what + " row_ws")
    _checkv(dsim.done(what), ref["dsim"], what + " dsim")
    empty = 1 if inp.counts is not None else P - 1
    assert float(loss.out[empty]) == 0.0 and not dsim.out[empty].any()


def test_smooth_ap_me_refuses_4097():
    """More keypoints than the row flags in LDS hold: the library's error from the host-side argument check, nothing launched, nothing written."""
    from gd_amd._lib import lib, ptr, stream
    N = 4097
    sim = torch.zeros(1, N, N, device="cuda")
    pts = torch.zeros(1, N, 3, device="cuda")
    dsim = torch.full((1, N, N), NAN, device="cuda")
    loss, rows = _Guarded((1,)), _Guarded((1, N, 2))
    rc = lib().gd_smooth_ap_me(ptr(sim), ptr(pts), ptr(pts), None, 1, N, 5e-3, 0.1, 0.01, ptr(loss.out), ptr(dsim), ptr(rows.out), stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"at most 4096" in lib().gd_last_error()
    assert torch.isnan(dsim).all() and torch.isnan(loss.buf).all() and torch.isnan(rows.buf).all()


# ------------------------------------------------------------------------------------------------ the step's glue
@pytest.mark.parametrize("view_major", [0, 1], ids=["pair_major", "view_major"])
def test_depth_bwd_combine(view_major):
    from gd_amd._lib import check, lib, ptr, stream
    du_r, du_l, hg_r, hg_l, g_l1, g_intra = L.combine_inputs()
    ref_du, ref_hg = L.combine(du_r, du_l, hg_r, hg_l, g_l1, g_intra, view_major)
    P, N = 3, 5
    dev = [t.cuda() for t in (du_r, du_l, hg_r, hg_l, g_l1, g_intra)]
    du, hg = _Guarded((2 * P * N, 128)), _Guarded((L.HG,))
    check(lib().gd_depth_bwd_combine(*[ptr(t) for t in dev], P, N, view_major, ptr(du.out), ptr(hg.out), stream()), "gd_depth_bwd_combine")
    what = f"gd_depth_bwd_combine view_major {view_major}"
    _checkv(du.done(what), ref_du, what + " du")
    _checkv(hg.done(what), ref_hg, what + " head gradients")


def test_scale_and_transpose():
    """One fp32 product per element, B = 2, R = 33, C = 65 (neither a multiple of the 32 x 32 tile): equal to the fp32 product, and its transpose."""
    from gd_amd._lib import check, lib, ptr, stream
    x, g = L.transpose_inputs()
    B, R, C = x.shape
    out, out_t = _Guarded((B, R, C)), _Guarded((B, C, R))
    xd, gd = x.cuda(), g.cuda()
    check(lib().gd_scale_and_transpose(ptr(xd), ptr(gd), ptr(out.out), ptr(out_t.out), B, R, C, stream()), "gd_scale_and_transpose")
    want = x * g[:, None, None]
    assert want.dtype == F32
    assert torch.equal(out.done("gd_scale_and_transpose").cpu(), want)
    assert torch.equal(out_t.done("gd_scale_and_transpose").cpu(), want.transpose(1, 2).contiguous())
