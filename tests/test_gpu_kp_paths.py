"""The keypoint sampling kernels (csrc/elementwise.hip: gd_kp_gather_fwd / _fwd_ln / _bwd / _bwd_det, gd_kp_patch_gather / _h, gd_kp_patch_bwd_det,
gd_kp_depth, gd_patch_mask) PER ELEMENT against the fp64 restatements of tests/kp_ref64.py: |got - ref64| <= bound(element), the bound derived there
from the kernel's operations, never measured; torch.equal where the inputs make every fp32 operation exact.  A failure reports the worst err / bound
and its index.  tests/test_kp_ref_host.py shows on the CPU that wrong references fail these bounds at these inputs.

Every kernel is called through lib() with its output inside a NaN-filled buffer: every element of the output must be written (the deterministic
scatters and the patch kernels write zeros too), the guard regions either side must keep their bits.  The parts of a token buffer a kernel has no
business reading (prefix rows, separator columns) are NaN as well.

Kernel, arm -> case:
  kp_gather_fwd_vec_kernel<float>   test_forward_gather[f32_vec8, f32_vec1032 (second trip of the channel loop), f32_tiny]
  kp_gather_fwd_vec_kernel<bf16>    test_forward_gather[bf16_vec8, bf16_vec1032]
  kp_gather_fwd_kernel (scalar)     by row size [f32_scalar6, bf16_scalar4, bf16_tiny], by misalignment [*_misaligned_grid, f32_misaligned_out],
                                    fp16 grids [f16_8, f16_6] (fp16 has no 16-byte kernel)
  kp_gather_fwd_ln_kernel<T>        test_forward_gather_ln[f32 | bf16]
  kp_gather_bwd_kernel              test_scatter[atomic-*];   kp_gather_bwd_det_kernel<float | bf16>   test_scatter[det_f32-* | det_bf16-*]
  kp_patch_gather_kernel<float, float | bf16, bf16 | float, f16>      test_patch_gather[f32 | bf16 | f16 - *]
  kp_patch_bwd_det_kernel<float, float | bf16, bf16>                  test_patch_backward[f32 | bf16 - *]"""
import pytest
import torch

import kp_ref64 as K

pytestmark = pytest.mark.gpu

BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16
GUARD = 64                    # elements either side of an output (a multiple of 16 bytes in every dtype)
SEAMS = [(n, False) for n in K.SCATTER_NK] + [(1024, True)]          # True: all 1024 keypoints inside one cell (a full LDS list)
SEAM_IDS = [f"{n}{'full' if f else ''}" for n, f in SEAMS]


def _check(got, ref, bound, what):
    """Every element: |got - ref| <= bound (bound 0: equality; a NaN anywhere fails)."""
    err = (got.detach().double() - ref.double()).abs()
    bound = bound.double().expand_as(err)
    ratio = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst, i = float(ratio.max()), int(ratio.argmax())
    idx = tuple(int(t) for t in torch.unravel_index(torch.tensor(i), ratio.shape))
    print(f"{what}: worst err / bound = {worst:.4f} at {idx}")
    assert worst <= 1.0, (f"{what}: worst err / bound = {worst:.3f} at {idx}: got {float(got.double().reshape(-1)[i])!r}, "
                          f"ref {float(ref.double().reshape(-1)[i])!r}, bound {float(bound.reshape(-1)[i]):.3e}")


def _bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


class _Guarded:
    """An output of `shape` inside a NaN-filled buffer, `shift` elements past 16-byte alignment."""

    def __init__(self, shape, dtype, shift=0):
        n = 1
        for s in shape:
            n *= s
        self.buf = torch.full((n + 2 * GUARD + shift,), float("nan"), dtype=dtype, device="cuda")
        self.before = _bits(self.buf).clone()
        self.lo, self.n = GUARD + shift, n
        self.out = self.buf[self.lo:self.lo + n].view(shape)

    def done(self, what, all_written=True):
        torch.cuda.synchronize()
        b = _bits(self.buf)
        assert torch.equal(b[:self.lo], self.before[:self.lo]) and torch.equal(b[self.lo + self.n:], self.before[self.lo + self.n:]), \
            f"{what}: wrote outside its output"
        if all_written:
            assert not torch.isnan(self.out).any(), f"{what}: left part of its output unwritten"
        return self.out


def _tokens(grid, prefix, pitch, shift=0, fill=float("nan")):
    """[B, gh, gw, D] -> (the view whose data_ptr is token 0 of the grid, bstride) of a token buffer [B, prefix + gh pitch, D], NaN in the prefix rows
    and separator columns, `shift` elements into its storage."""
    B, gh, gw, D = grid.shape
    rows = prefix + gh * pitch
    flat = torch.full((B * rows * D + shift,), fill, dtype=grid.dtype, device="cuda")
    buf = flat[shift:].view(B, rows, D)
    buf[:, prefix:].view(B, gh, pitch, D)[:, :, :gw] = grid.cuda()
    return buf[:, prefix:], rows * D


def _geom_args(geom):
    return (float(geom["sx"]), float(geom["sy"]), geom["img_h"], geom["img_w"], geom["patch"], geom["stride"])


def _fwd_arm(grids, out, D, bstride):
    """The predicate of gd_kp_gather_fwd."""
    es = grids[0].element_size()
    vec = (grids[0].dtype in (F32, BF) and (D * es) % 16 == 0 and (bstride * es) % 16 == 0 and out.data_ptr() % 16 == 0 and D % 4 == 0
           and all(g.data_ptr() % 16 == 0 for g in grids))
    return "scalar" if not vec else "vec_bf16" if grids[0].dtype == BF else "vec_f32"


def _gather_fwd(geom, kp, grids, prefix, pitch, shift_grid=0, shift_out=0, expect=None):
    from gd_amd._lib import check, dtype_code, lib, ptr, stream
    from gd_amd.ops import _ptr_array
    B, Nk = kp.shape[:2]
    gh, gw, D = geom["gh"], geom["gw"], grids[0].shape[-1]
    views = [_tokens(g, prefix, pitch, shift_grid) for g in grids]
    toks, bstride = [v[0] for v in views], views[0][1]
    o = _Guarded((B, Nk, D), F32, shift_out)
    if expect is not None:
        assert _fwd_arm(toks, o.out, D, bstride) == expect, "the case does not reach the dispatch arm it is there for"
    kq = kp.cuda()
    check(lib().gd_kp_gather_fwd(_ptr_array(toks), len(toks), bstride, dtype_code(toks[0]), ptr(kq), ptr(o.out), B, Nk, gh, gw, D, *_geom_args(geom),
                                 pitch, stream()), "gd_kp_gather_fwd")
    return o.done("gd_kp_gather_fwd")


# ------------------------------------------------------------------------------------------------ forward gathers
@pytest.mark.parametrize("case", K.FWD_CASES, ids=[c[0] for c in K.FWD_CASES])
def test_forward_gather(case):
    name, _, dtype, D, ngrid, extra, prefix, mis = case
    geom, kp, grids = K.fwd_inputs(case)
    expect = "vec_bf16" if name.startswith("bf16_vec") else "vec_f32" if name in ("f32_vec8", "f32_vec1032", "f32_tiny") else "scalar"
    got = _gather_fwd(geom, kp, grids, prefix, geom["gw"] + extra, shift_grid=1 if mis == "grid" else 0, shift_out=1 if mis == "out" else 0,
                      expect=expect)
    W, dW = K.geometry64(kp.cuda(), geom)
    g = [t.cuda() for t in grids]
    _check(got, K.gather_fwd64(g, W), K.gather_fwd_bound(g, W, dW), f"kp_gather_fwd {name}")


@pytest.mark.parametrize("ngrid", [1, 2, 4])
@pytest.mark.parametrize("dtype,D", [(F32, 8), (F32, 6), (BF, 8), (F16, 8)], ids=["f32_vec", "f32_scalar", "bf16_vec", "f16"])
def test_forward_gather_exact(dtype, D, ngrid):
    """The exact geometry, keypoints in quarters of a cell, integer grid values up to 64, a power-of-two ngrid: every weight is a multiple of 1 / 16 and
    every product and sum is exact in fp32 — the result must EQUAL the fp64 one."""
    geom = K.GEOMS["exact"]
    kp, gx, gy = K.exact_keypoints(geom, 2, 48, 5)
    gen = torch.Generator().manual_seed(6)
    grids = [torch.randint(-64, 65, (2, geom["gh"], geom["gw"], D), generator=gen).to(dtype) for _ in range(ngrid)]
    got = _gather_fwd(geom, kp, grids, 1, geom["gw"] + 1)
    W = K.weights64(gx, gy, geom["gh"], geom["gw"]).cuda()
    assert torch.equal(got.double(), K.gather_fwd64([g.cuda() for g in grids], W))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_forward_gather_ln(dtype):
    """gd_kp_gather_fwd_ln with a prefix token, a pitched grid, rows of large mean and 1 / sigma from 2^-6 to 2^6 (the statistics are the kernel's
    inputs: the reference normalises with exactly these)."""
    from gd_amd._lib import check, dtype_code, lib, ptr, stream
    from gd_amd.ops import _ptr_array
    geom = K.GEOMS["generic"]
    gh, gw, D, B, Nk, ngrid, prefix, pitch = geom["gh"], geom["gw"], 16, 2, K.FWD_NK, 3, 1, geom["gw"] + 1
    kp = K.probe_keypoints(geom, B, Nk, 41)
    gen = torch.Generator().manual_seed(42)
    grids, means, rstds = [], [], []
    for t in range(ngrid):
        rs = torch.exp2(torch.rand(B, gh, gw, generator=gen) * 12 - 6)
        mu = torch.randn(B, gh, gw, generator=gen) * torch.where(torch.rand(B, gh, gw, generator=gen) < 0.3, 1e3, 1.0)
        grids.append((mu[..., None] + torch.randn(B, gh, gw, D, generator=gen) / rs[..., None]).to(dtype))
        means.append(mu)
        rstds.append(rs)
    gm, bt = torch.randn(D, generator=gen).cuda(), torch.randn(D, generator=gen).cuda()
    views = [_tokens(g, prefix, pitch) for g in grids]
    toks, bstride = [v[0] for v in views], views[0][1]
    mv = [_tokens(m[..., None], prefix, pitch)[0] for m in means]
    rv = [_tokens(r[..., None], prefix, pitch)[0] for r in rstds]
    o = _Guarded((B, Nk, D), F32)
    kq = kp.cuda()
    check(lib().gd_kp_gather_fwd_ln(_ptr_array(toks), _ptr_array(mv), _ptr_array(rv), ngrid, bstride, prefix + gh * pitch, dtype_code(toks[0]),
                                    ptr(gm), ptr(bt), ptr(kq), ptr(o.out), B, Nk, gh, gw, D, *_geom_args(geom), pitch, stream()),
          "gd_kp_gather_fwd_ln")
    got = o.done("gd_kp_gather_fwd_ln")
    W, dW = K.geometry64(kq, geom)
    g, m, r = [t.cuda() for t in grids], [t.cuda() for t in means], [t.cuda() for t in rstds]
    _check(got, K.gather_ln_fwd64(g, m, r, gm, bt, W), K.gather_ln_fwd_bound(g, m, r, gm, bt, W, dW), f"kp_gather_fwd_ln {dtype}")


# ------------------------------------------------------------------------------------------------ scatters
def _bwd_det(geom, kp, dout, scale, dtype, prefix, pitch):
    from gd_amd._lib import check, dtype_code, lib, ptr, stream
    B, Nk, D = dout.shape
    gh, gw = geom["gh"], geom["gw"]
    rows = prefix + gh * pitch
    o = _Guarded((B, rows, D), dtype)
    check(lib().gd_kp_gather_bwd_det(ptr(o.out), dtype_code(o.out), rows * D, prefix, ptr(kp), ptr(dout), float(scale), B, Nk, gh, gw, D,
                                     *_geom_args(geom), pitch, stream()), "gd_kp_gather_bwd_det")
    return o.done("gd_kp_gather_bwd_det")


def _layout(i, gw):
    """pitch in {gw, gw + 1} x prefix in {0, 1}, by case number."""
    return i % 2, gw + (i // 2) % 2


SCATTER_D = {1: 1024, 63: 8, 64: 40, 65: 1024, 256: 8, 257: 40, 1024: 8}


@pytest.mark.parametrize("Nk,full", SEAMS, ids=SEAM_IDS)
@pytest.mark.parametrize("kind", ["det_f32", "det_bf16", "atomic"])
def test_scatter(kind, Nk, full):
    """Both interpolate_features backwards against gather_bwd64 (not against each other), across the ballot (64) and scan (256) seams of the
    keypoint compaction and with a full LDS list; prefix rows and separator columns exactly zero; the deterministic one bit-identical twice."""
    from gd_amd import ops
    i = SEAMS.index((Nk, full))
    gname = "exact" if i % 2 else "generic"
    D = SCATTER_D[Nk]
    geom, kp, dout = K.scatter_inputs(gname, Nk, D, full=full)
    gh, gw = geom["gh"], geom["gw"]
    prefix, pitch = _layout(i, gw)
    kp, dout = kp.cuda(), dout.cuda()
    W, dW = K.geometry64(kp, geom)
    a = (float(geom["sx"]), float(geom["sy"]), geom["img_h"], geom["img_w"], geom["patch"])
    if kind == "atomic":
        ngrid = 1 + i % 3
        outs = ops.kp_gather_bwd(ngrid, kp, dout, 2, Nk, gh, gw, D, *a, prefix=prefix, pitch=pitch)
        ref = K.gather_bwd64(dout, W, 1.0 / ngrid, prefix, pitch)
        bound = K.gather_bwd_bound(dout, W, dW, 1.0 / ngrid, F32, True, prefix, pitch)
        assert len(outs) == ngrid
        for t, got in enumerate(outs):
            _check(got, ref, bound, f"kp_gather_bwd Nk {Nk} grid {t}")
        return
    dtype = F32 if kind == "det_f32" else BF
    scale = K._f32(0.37)
    got = _bwd_det(geom, kp, dout, scale, dtype, prefix, pitch)
    again = ops.kp_gather_bwd_det(kp, dout, scale, dtype, 2, Nk, gh, gw, D, *a, prefix=prefix, pitch=pitch)
    assert again is not None and torch.equal(_bits(got), _bits(again)), "two runs of the deterministic scatter differ"
    _check(got, K.gather_bwd64(dout, W, scale, prefix, pitch), K.gather_bwd_bound(dout, W, dW, scale, dtype, False, prefix, pitch),
           f"kp_gather_bwd_det {kind} Nk {Nk}")
    assert not got[:, :prefix].any() and not got[:, prefix:].view(2, gh, pitch, D)[:, :, gw:].any()


@pytest.mark.parametrize("kind", ["det_f32", "det_bf16", "atomic"])
def test_scatter_exact_one_hot(kind):
    """The exact geometry, keypoints in quarters, keypoint k's gradient 1 in channel k alone and a power-of-two scale: channel k of the result is
    scale W[k], its (up to) four weights on exactly their cells with exactly their values, zero everywhere else."""
    from gd_amd import ops
    geom = K.GEOMS["exact"]
    gh, gw, Nk = geom["gh"], geom["gw"], 40
    kp, gx, gy = K.exact_keypoints(geom, 2, Nk, 7)
    dout = torch.eye(Nk).expand(2, Nk, Nk).contiguous().cuda()
    W = K.weights64(gx, gy, gh, gw).cuda()
    ref = K.gather_bwd64(dout, W, 0.5, 1, gw + 1)
    assert int((ref != 0).sum()) == int((W != 0).sum())
    if kind == "atomic":
        outs = ops.kp_gather_bwd(2, kp.cuda(), dout, 2, Nk, gh, gw, Nk, 1.0, 1.0, geom["img_h"], geom["img_w"], 16, prefix=1, pitch=gw + 1)
        assert all(torch.equal(o.double(), ref) for o in outs)
    else:
        got = _bwd_det(geom, kp.cuda(), dout, 0.5, F32 if kind == "det_f32" else BF, 1, gw + 1)
        assert torch.equal(got.double(), ref)


def test_scatter_refusals_stay_refusals():
    """Outside the deterministic kernel's range the wrapper returns None (the caller then takes the atomic scatter); the C entry point refuses."""
    from gd_amd import ops
    from gd_amd._lib import dtype_code, lib, ptr, stream
    geom = K.GEOMS["exact"]
    a = (1.0, 1.0, geom["img_h"], geom["img_w"], 16)
    for Nk, D in ((1025, 8), (4, 12), (4, 1032)):
        kp = torch.zeros(1, Nk, 2, device="cuda")
        dout = torch.zeros(1, Nk, D, device="cuda")
        assert ops.kp_gather_bwd_det(kp, dout, 1.0, F32, 1, Nk, 5, 9, D, *a) is None
        o = _Guarded((1, 45, D), F32)
        rc = lib().gd_kp_gather_bwd_det(ptr(o.out), dtype_code(o.out), 45 * D, 0, ptr(kp), ptr(dout), 1.0, 1, Nk, 5, 9, D, *_geom_args(geom), 9, stream())
        assert rc != 0
        assert torch.isnan(o.done("gd_kp_gather_bwd_det (refused)", all_written=False)).all()


# ------------------------------------------------------------------------------------------------ 3x3 patches at the keypoints
def _patch_gather(geom, kp, grid, out_dtype, prefix, pitch):
    from gd_amd._lib import check, dtype_code, lib, ptr, stream
    B, Nk = kp.shape[:2]
    gh, gw, D = geom["gh"], geom["gw"], grid.shape[-1]
    tok, bstride = _tokens(grid, prefix, pitch)
    o = _Guarded((B * Nk, 9 * D), out_dtype)
    if out_dtype == F16:
        check(lib().gd_kp_patch_gather_h(ptr(tok), bstride, ptr(kp), ptr(o.out), B, Nk, gh, gw, D, *_geom_args(geom), pitch, stream()),
              "gd_kp_patch_gather_h")
    else:
        check(lib().gd_kp_patch_gather(ptr(tok), bstride, dtype_code(tok), ptr(kp), ptr(o.out), B, Nk, gh, gw, D, *_geom_args(geom), pitch,
                                       stream()), "gd_kp_patch_gather")
    return o.done("gd_kp_patch_gather")


def _patch_bwd(geom, kp, U9, dtype, prefix):
    from gd_amd._lib import check, dtype_code, lib, ptr, stream
    B, Nk = kp.shape[:2]
    gh, gw, D = geom["gh"], geom["gw"], U9.shape[-1] // 9
    Nt = prefix + gh * gw
    o = _Guarded((B, Nt, D), dtype)
    check(lib().gd_kp_patch_bwd_det(ptr(U9), ptr(o.out), dtype_code(o.out), Nt * D, prefix, ptr(kp), B, Nk, gh, gw, D, *_geom_args(geom), stream()),
          "gd_kp_patch_bwd_det")
    return o.done("gd_kp_patch_bwd_det")


PATCH_D = {1: 1024, 65: 1024}          # every other list length: D = 8


@pytest.mark.parametrize("Nk,full", SEAMS, ids=SEAM_IDS)
@pytest.mark.parametrize("pair", ["f32", "bf16", "f16"])
def test_patch_gather(pair, Nk, full):
    """gd_kp_patch_gather (f32 -> f32, bf16 -> bf16) and gd_kp_patch_gather_h (f32 -> fp16); probe_keypoints sits in every corner and edge cell, so
    the rows and columns -1 and g of the 4 x 4 footprint are read as the zero ring."""
    i = SEAMS.index((Nk, full))
    gname = "generic" if i % 2 else "exact"
    tin, tout = {"f32": (F32, F32), "bf16": (BF, BF), "f16": (F32, F16)}[pair]
    geom, kp, grid, _ = K.patch_inputs(gname, Nk, PATCH_D.get(Nk, 8), tin, full=full)
    prefix, pitch = _layout(i, geom["gw"])
    kp, grid = kp.cuda(), grid.cuda()
    got = _patch_gather(geom, kp, grid, tout, prefix, pitch)
    W, dW = K.geometry64(kp, geom)
    _check(got, K.patch_gather64(grid, W), K.patch_gather_bound(grid, W, dW, tout), f"kp_patch_gather {pair} Nk {Nk}")


def test_patch_gather_fp16_taps_saturate():
    """Taps just above 65504 leave as +-65504, never as inf: against patch_gather64 clamped to the fp16 range."""
    geom = K.GEOMS["generic"]
    kp = K.probe_keypoints(geom, 2, 48, 43).cuda()
    gen = torch.Generator().manual_seed(44)
    grid = (65504.0 + torch.rand(2, geom["gh"], geom["gw"], 8, generator=gen) * 200 - 40) * torch.where(torch.rand(2, 1, 1, 8, generator=gen) < 0.5, -1.0, 1.0)
    grid = grid.cuda()
    got = _patch_gather(geom, kp, grid, F16, 0, geom["gw"])
    W, dW = K.geometry64(kp, geom)
    ref = K.patch_gather64(grid, W)
    assert (ref.abs() > 65520).any() and torch.isfinite(got).all() and float(got.abs().max()) == 65504.0
    _check(got, ref.clamp(-65504.0, 65504.0), K.patch_gather_bound(grid, W, dW, F16), "kp_patch_gather_h saturating")


@pytest.mark.parametrize("Nk,full", SEAMS, ids=SEAM_IDS)
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_patch_backward(dtype, Nk, full):
    i = SEAMS.index((Nk, full))
    gname = "exact" if i % 2 else "generic"
    geom, kp, _, U9 = K.patch_inputs(gname, Nk, PATCH_D.get(Nk, 8), dtype, full=full)
    prefix = (i // 2) % 2
    kp, U9 = kp.cuda(), U9.cuda()
    got = _patch_bwd(geom, kp, U9, dtype, prefix)
    assert torch.equal(_bits(got), _bits(_patch_bwd(geom, kp, U9, dtype, prefix))), "two runs of the deterministic patch backward differ"
    W, dW = K.geometry64(kp, geom)
    _check(got, K.patch_bwd64(U9, W, prefix), K.patch_bwd_bound(U9, W, dW, dtype, prefix), f"kp_patch_bwd_det {dtype} Nk {Nk}")
    assert not got[:, :prefix].any()


@pytest.mark.parametrize("pair", ["f32", "bf16", "f16"])
def test_patch_kernels_exact(pair):
    """The exact geometry, keypoints in quarters, small integer values: every tap (and, in fp32, every token gradient) is exact."""
    geom = K.GEOMS["exact"]
    gh, gw, Nk, D = geom["gh"], geom["gw"], 40, 8
    tin, tout = {"f32": (F32, F32), "bf16": (BF, BF), "f16": (F32, F16)}[pair]
    kp, gx, gy = K.exact_keypoints(geom, 2, Nk, 9)
    W = K.weights64(gx, gy, gh, gw).cuda()
    gen = torch.Generator().manual_seed(10)
    lim = 4 if pair == "bf16" else 64                   # a tap is a multiple of 1 / 16 up to lim: 6 significant bits for bf16's 8
    grid = torch.randint(-lim, lim + 1, (2, gh, gw, D), generator=gen).to(tin).cuda()
    assert torch.equal(_patch_gather(geom, kp.cuda(), grid, tout, 1, gw + 1).double(), K.patch_gather64(grid, W))
    if pair == "f32":
        U9 = torch.randint(-4, 5, (2 * Nk, 9 * D), generator=gen).float().cuda()
        assert torch.equal(_patch_bwd(geom, kp.cuda(), U9, F32, 1).double(), K.patch_bwd64(U9, W, 1))


def test_patch_gather_refuses_fp16_grids():
    """gd_kp_patch_gather has f32 and bf16 kernels only: an fp16 grid is an error from the wrapper and from the C entry point, which launches nothing."""
    from gd_amd import ops
    from gd_amd._lib import GdHipError, dtype_code, lib, ptr, stream
    geom = K.GEOMS["exact"]
    gh, gw = geom["gh"], geom["gw"]
    kp = K.probe_keypoints(geom, 1, 4, 1).cuda()
    grid = torch.zeros(1, gh * gw, 8, dtype=F16, device="cuda")
    with pytest.raises(GdHipError):
        ops.kp_patch_gather(grid, gh * gw * 8, kp, 1, 4, gh, gw, 8, 1.0, 1.0, geom["img_h"], geom["img_w"], 16)
    o = _Guarded((4, 72), F16)
    rc = lib().gd_kp_patch_gather(ptr(grid), gh * gw * 8, dtype_code(grid), ptr(kp), ptr(o.out), 1, 4, gh, gw, 8, *_geom_args(geom), gw, stream())
    assert rc != 0 and b"f32 or bf16" in lib().gd_last_error()
    assert torch.isnan(o.done("gd_kp_patch_gather (refused)", all_written=False)).all()


# ------------------------------------------------------------------------------------------------ depth at keypoints, patch mask
def test_kp_depth():
    """7 x 10 depth maps; keypoints at (0, 0) and (W - 1, H - 1), -1-padded, beyond the image, fractional (y in quarters: y W is exact in fp32
    whether or not the kernel fuses y W + x)."""
    from gd_amd import ops
    H, Wd, B = 7, 10, 2
    gen = torch.Generator().manual_seed(50)
    depth = torch.rand(B, H, Wd, generator=gen) * 9 + 0.5
    depth[1] -= 5.0                                                         # mixed signs: the bound goes with the mean magnitude
    kp = torch.stack([torch.randint(0, 4 * Wd, (B, 40), generator=gen) / 4.0, torch.randint(0, 4 * H, (B, 40), generator=gen) / 4.0], -1)
    kp[:, 0], kp[:, 1], kp[:, 2] = torch.tensor([0.0, 0.0]), torch.tensor([Wd - 1.0, H - 1.0]), torch.tensor([-1.0, -1.0])
    kp[:, 3], kp[:, 4], kp[:, 5] = torch.tensor([1e4, 3.0]), torch.tensor([3.0, 1e4]), torch.tensor([-500.0, 2.0])
    kp[1, 30:] = -1.0
    depth, kp = depth.cuda(), kp.cuda()
    got = ops.kp_depth(depth, kp)
    _check(got, K.kp_depth64(depth, kp), K.kp_depth_bound(depth, kp), "kp_depth")


def test_patch_mask():
    """Exact equality; H, W no multiples of P with keypoints in the remainder strip; x = W - 0.5 (inside), x = W and x = -0.5 (outside); duplicates;
    an all-padding batch row gives an all-zero mask."""
    from gd_amd import ops
    H, Wd, P = 45, 60, 14
    gen = torch.Generator().manual_seed(51)
    kp = torch.rand(3, 300, 2, generator=gen) * torch.tensor([Wd + 10.0, H + 10.0]) - 5
    kp[0, :8] = torch.tensor([[Wd - 0.5, 3.0], [float(Wd), 3.0], [-0.5, 3.0], [57.0, 20.0], [20.0, 43.5], [13.9, 41.9], [13.9, 41.9], [55.99, 41.99]])
    kp[0, 8:, 0] *= 0.4                                                      # row 0 leaves the right-hand patches to the keypoints above
    kp[1, 10:] = kp[1, :10].repeat(29, 1)
    kp[2] = -1.0
    kp = kp.cuda()
    got = ops.patch_mask(kp, H, Wd, P)
    ref = K.patch_mask_ref(kp, H, Wd, P)
    assert got.dtype == torch.uint8 and torch.equal(got, ref)
    assert ref[0].any() and not ref[0].all() and not got[2].any()
    kp2 = torch.rand(2, 50, 2, generator=gen).cuda() * torch.tensor([70.0, 56.0], device="cuda")
    assert torch.equal(ops.patch_mask(kp2, 56, 70, 14), K.patch_mask_ref(kp2, 56, 70, 14))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_two_by_two_grid_scatters_and_patches(dtype):
    """gh = gw = 2: every clamped neighbour coincides with a node and every 4 x 4 footprint reaches the zero ring on all four sides."""
    from gd_amd import ops
    geom, kp, grid, U9 = K.patch_inputs("tiny", K.FWD_NK, 8, dtype)
    _, _, dout = K.scatter_inputs("tiny", K.FWD_NK, 8)
    kp, grid, U9, dout = kp.cuda(), grid.cuda(), U9.cuda(), dout.cuda()
    W, dW = K.geometry64(kp, geom)
    scale = K._f32(1.7)
    _check(_bwd_det(geom, kp, dout, scale, dtype, 1, 3), K.gather_bwd64(dout, W, scale, 1, 3),
           K.gather_bwd_bound(dout, W, dW, scale, dtype, False, 1, 3), f"kp_gather_bwd_det 2x2 {dtype}")
    if dtype == F32:
        got = ops.kp_gather_bwd(2, kp, dout, 2, K.FWD_NK, 2, 2, 8, 1.0, 1.0, 32, 32, 16, prefix=1, pitch=3)
        for t in range(2):
            _check(got[t], K.gather_bwd64(dout, W, 0.5, 1, 3), K.gather_bwd_bound(dout, W, dW, 0.5, F32, True, 1, 3), "kp_gather_bwd 2x2")
    _check(_patch_gather(geom, kp, grid, dtype, 1, 3), K.patch_gather64(grid, W), K.patch_gather_bound(grid, W, dW, dtype), f"kp_patch_gather 2x2 {dtype}")
    if dtype == F32:
        _check(_patch_gather(geom, kp, grid, F16, 0, 2), K.patch_gather64(grid, W), K.patch_gather_bound(grid, W, dW, F16), "kp_patch_gather_h 2x2")
    _check(_patch_bwd(geom, kp, U9, dtype, 1), K.patch_bwd64(U9, W, 1), K.patch_bwd_bound(U9, W, dW, dtype, 1), f"kp_patch_bwd_det 2x2 {dtype}")
