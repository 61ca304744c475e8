"""Self-attention forward / backward (csrc/attention.hip) PER ELEMENT against the fp64 restatement of tests/attn_ref64.py: |got - ref64| <= bound(element)
for o, lse, dq, dk and dv separately, the bound derived there from the kernel's operation order, never measured; three input families (random, the
uniform-count probe, the pair-selector probe: attn_ref64.make_inputs) whose probes turn a missed or doubled key, query or tile into an O(1) error in a
named row (tests/test_attn_ref_host.py shows that every such mutant of the restatement violates these bounds by a factor >= 4).  Also: a (b, h) slice of a
batched call is bit-identical to the one-head call; two runs are bit-identical; the column-order / dV-only / power-of-two contracts; and nothing outside
the logical arrays is read or written (NaN canaries, a NaN-filled workspace of exactly gd_attention_bwd_workspace_bytes).  A failure reports the worst
err / bound, the output and (b, h, row, column).  With GD_ATTN_ERRORS=<file> the worst ratio of every (path, dtype, family, output) group is written
there (profiles/attention_errors.txt).

Kernel templates and instantiations named by the launch sites (attn_fwd_launch, attn_dkv_launch, attn_bwd_launch) and the case that reaches each
(profiles/attention_path_coverage.txt has the table with the sizes):
  attn_fwd_kernel<float | x3>                    test_bounds[f32 | x3 - N], path default
  attn_fwd_kernel<bf16 | f16>                    test_bounds[bf16 | f16 - N], path attn_dma=0
  attn_fwd_dma_kernel<bf16 | f16>                test_bounds[bf16 | f16 - N], path default (rotated key order), path attn_rot=0 (plain order);
                                                 nfull = 0 .. 11: nsteady 0, 3, 6, 9 with 0, 1, 2 generic full tiles, tails 0 / 1 / 63, the wrap inside
                                                 the steady loop from N = 321; test_long_sweeps: 62 and 64 full tiles
  attn_bwd_dq_kernel<float | x3>                 test_bounds[f32 | x3 - N], path default
  attn_bwd_dq_kernel<bf16 | f16>                 test_bounds[bf16 | f16 - N], path attn_dq_dma=0
  attn_bwd_dq_dma_kernel<bf16 | f16>             test_bounds[bf16 | f16 - N], path default
  attn_bwd_dkv_kernel<float, 8, true>            test_bounds[f32 - N] (need_dk=False runs the same instantiation)
  attn_bwd_dkv_kernel<x3, 4, true | false>       test_bounds[x3 - N]: need_dk True | False
  attn_bwd_dkv_kernel<bf16 | f16, 4, DK>         test_bounds[.. - N], path attn_dkv_dma=0, N % 256 in 1 .. 128 (1, 3, 17, 63, 64, 65, 127, 128, 257, 321, 383, 384, 513, 577)
  attn_bwd_dkv_kernel<bf16 | f16, 8, DK>         test_bounds[.. - N], path default at the other N (129 .. 256, 385, 449, 705), path attn_dkv_nw=8 at every N;
                                                 test_long_sweeps[.. - 4097] (N >= 4096)
  attn_bwd_dkv_dma_kernel<bf16 | f16, DK>        test_bounds[.. - N], path default at N % 256 in 1 .. 128, path attn_dkv_nw=4 at every N; test_long_sweeps[.. - 3968]
  (DK = false: every path's need_dk=False run, held bit-identical in dq and dv to its need_dk=True run)"""
import os

import pytest
import torch

import attn_ref64 as R

pytestmark = pytest.mark.gpu

GRID = [1, 3, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 321, 383, 384, 385, 449, 513, 577, 705]
# the random family is the thinned one (tests/test_gpu_attention.py already runs it at its own sizes): sizes on both sides of every dK/dV form and tile path;
# the two probes run at every size
RANDOM_N = [1, 3, 17, 63, 129, 257, 449, 705]
KINDS = list(R.KINDS)
SIXTEEN = ["bf16", "f16"]
OPTION_DEFAULTS = {"attn_dma": 1, "attn_rot": 1, "attn_dq_dma": 1, "attn_dkv_dma": 1, "attn_dkv_nw": 0}
FWD_OPTIONS = [("attn_dma", 0), ("attn_rot", 0)]                                           # change the forward kernel only
BWD_OPTIONS = [("attn_dq_dma", 0), ("attn_dkv_dma", 0), ("attn_dkv_nw", 4), ("attn_dkv_nw", 8)]      # change a backward kernel only
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GD_ATTN_ERRORS")
    if path and _WORST:
        with open(path, "w") as f:
            for k in sorted(_WORST):
                f.write(f"{_WORST[k][0]:8.4f}  {k:44s} worst at {_WORST[k][1]}\n")


class _option:
    """One library option off its default for the duration of a `with` block."""

    def __init__(self, name=None, value=None):
        self.name, self.value = name, value

    def __enter__(self):
        from gd_amd._lib import check, lib
        if self.name is not None:
            assert lib().gd_debug_get(self.name.encode()) == OPTION_DEFAULTS[self.name], f"{self.name} is not at its default"
            check(lib().gd_debug_set(self.name.encode(), self.value), "gd_debug_set")
            assert lib().gd_debug_get(self.name.encode()) == self.value

    def __exit__(self, *exc):
        from gd_amd._lib import lib
        if self.name is not None:
            lib().gd_debug_set(self.name.encode(), OPTION_DEFAULTS[self.name])
            assert lib().gd_debug_get(self.name.encode()) == OPTION_DEFAULTS[self.name]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _fwd(qkv, B, N, H, kind):
    from gd_amd import ops
    return ops.attention_fwd(qkv, B, N, H, x3=(kind == "x3"))


def _bwd(qkv, o, dout, lse, B, N, H, kind, **kw):
    from gd_amd import ops
    return ops.attention_bwd(qkv, o, dout, lse, B, N, H, x3=(kind == "x3"), **kw)


def _check(group, what, got, ref, bound, tag):
    worst, idx = R.ratio(got, ref, bound)
    key = f"{group} {what}"
    if worst > _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (worst, f"{tag} (b, h, row, col) = {idx}")
    assert worst <= 1.0, (f"{group} / {what} / {tag}: worst err / bound = {worst:.3f} at (b, h, row[, col]) = {idx}: got {float(got[idx])!r}, "
                          f"ref {float(ref[idx])!r}, bound {float(bound[idx]):.3e}")


def _check_fwd(path, kind, family, tag, o, lse, fref, B, N, H):
    ro, rl, bo, bl = fref
    _check(f"{path} {kind} {family}", "o", R.heads_o(o, B, N, H), ro, bo, tag)
    _check(f"{path} {kind} {family}", "lse", lse.double().cpu(), rl, bl, tag)


def _check_bwd(path, kind, family, tag, dqkv, bref, B, N, H):
    for what, got, ref, bound in zip(("dq", "dk", "dv"), R.heads(dqkv, B, N, H), bref[:3], bref[3:]):
        _check(f"{path} {kind} {family}", what, got, ref, bound, tag)
    if family == "uniform":      # q = 0: dk = dS^T q / 8 is exactly zero
        assert float(R.heads(dqkv, B, N, H)[1].abs().max()) == 0.0, f"{path} {kind} uniform {tag}: dk != 0"


def _run_family(kind, family, B, N, H, with_options):
    """The default path of one (dtype, size, family) against its fp64 reference, run twice (determinism), and — 16-bit types, probes — every
    option-only path against the SAME reference: a forward option feeds nothing into the comparison but its own o and lse; a backward option runs on the
    default forward's o and lse, the ones the backward reference was built from."""
    tag = f"B={B} N={N} H={H}"
    qkv_c, dout_c = R.make_inputs(family, B, N, H, kind)
    qkv, dout = qkv_c.cuda(), dout_c.cuda()
    q, k, v = R.heads(qkv_c, B, N, H)
    do = R.heads_o(dout_c, B, N, H)
    fref = R.uniform_fwd(v, kind) if family == "uniform" else R.fwd_bound(q, k, v, kind)
    o, lse = _fwd(qkv, B, N, H, kind)
    dqkv = _bwd(qkv, o, dout, lse, B, N, H, kind)
    o2, lse2 = _fwd(qkv, B, N, H, kind)
    assert _same(o, o2) and _same(lse, lse2) and _same(dqkv, _bwd(qkv, o2, dout, lse2, B, N, H, kind)), f"{kind} {family} {tag}: two runs differ"
    _check_fwd("default", kind, family, tag, o, lse, fref, B, N, H)
    bref = R.bwd_bound(q, k, v, R.heads_o(o, B, N, H), lse.double().cpu(), do, kind)      # the backward of the GIVEN o, lse
    _check_bwd("default", kind, family, tag, dqkv, bref, B, N, H)
    D = H * 64
    d3 = _bwd(qkv, o, dout, lse, B, N, H, kind, need_dk=False)
    assert _same(d3[:, :D], dqkv[:, :D]) and _same(d3[:, 2 * D:], dqkv[:, 2 * D:]), f"{kind} {family} {tag}: need_dk=False changes dq or dv"
    if not with_options:
        return
    for name, val in FWD_OPTIONS:
        with _option(name, val):
            oo, ol = _fwd(qkv, B, N, H, kind)
        _check_fwd(f"{name}={val}", kind, family, tag, oo, ol, fref, B, N, H)
    for name, val in BWD_OPTIONS:
        with _option(name, val):
            dd = _bwd(qkv, o, dout, lse, B, N, H, kind)
            d3 = _bwd(qkv, o, dout, lse, B, N, H, kind, need_dk=False)
        _check_bwd(f"{name}={val}", kind, family, tag, dd, bref, B, N, H)
        assert _same(d3[:, :D], dd[:, :D]) and _same(d3[:, 2 * D:], dd[:, 2 * D:]), f"{name}={val} {kind} {family} {tag}: need_dk=False changes dq or dv"


@pytest.mark.parametrize("N", GRID)
@pytest.mark.parametrize("kind", KINDS)
def test_bounds(kind, N):
    """B = 2, H = 2 over the size grid: nfull = 0 .. 11 (nsteady 0, 3, 6, 9 and 0 - 2 generic full tiles behind the steady loop), tails 0 / 1 / 63, one
    to six x-blocks, the rotation wrap inside the steady loop from N = 321, N % 256 in {0, 1, 127, 128, 129, 255}."""
    for family in R.FAMILIES:
        if family == "random" and N not in RANDOM_N:
            continue
        _run_family(kind, family, 2, N, 2, with_options=(kind in SIXTEEN and family != "random"))


@pytest.mark.parametrize("N", [3968, 4097])
@pytest.mark.parametrize("kind", SIXTEEN)
def test_long_sweeps(kind, N):
    """One head: 3968 = 62 full tiles, N % 256 = 128, below 4096 -> the four-wave LDS-DMA dK/dV form on a long sweep; 4097 = 64 full tiles + a
    one-key tail, at the 4096 threshold of attn_dkv_form -> the eight-wave form."""
    for family in ("uniform", "pair"):
        _run_family(kind, family, 1, N, 1, with_options=False)


@pytest.mark.parametrize("N", [193, 385])
@pytest.mark.parametrize("kind", KINDS)
def test_slice_equals_single_head_call(kind, N):
    """Nothing in a block's arithmetic depends on b or h (attn_block_coords renames blocks, the rotation is (2 xb) % nfull): head (b, h) of a
    B = 2, H = 3 call is bit-identical to the B = 1, H = 1 call on that head's columns — o, lse and all three gradients."""
    B, H = 2, 3
    qkv_c, dout_c = R.make_inputs("pair", B, N, H, kind)
    qkv, dout = qkv_c.cuda(), dout_c.cuda()
    o, lse = _fwd(qkv, B, N, H, kind)
    dqkv = _bwd(qkv, o, dout, lse, B, N, H, kind)
    x, g, oo, dd = qkv.view(B, N, 3, H, 64), dqkv.view(B, N, 3, H, 64), o.view(B, N, H, 64), dout.view(B, N, H, 64)
    for b in range(B):
        for h in range(H):
            q1 = x[b, :, :, h].reshape(N, 192).contiguous()
            d1 = dd[b, :, h].contiguous()
            o1, l1 = _fwd(q1, 1, N, 1, kind)
            assert _same(o1, oo[b, :, h]) and _same(l1.view(N), lse[b, h]), f"{kind} N={N}: forward of head ({b}, {h})"
            g1 = _bwd(q1, o1, d1, l1, 1, N, 1, kind)
            assert _same(g1, g[b, :, :, h].reshape(N, 192)), f"{kind} N={N}: backward of head ({b}, {h})"


@pytest.mark.parametrize("N", [17, 65, 193])
@pytest.mark.parametrize("kind", KINDS)
def test_contracts(kind, N):
    """vfirst exchanges the dK and dV column blocks exactly; need_dk=False leaves dq and dv bit-identical (with and without vfirst)."""
    B, H, D = 2, 2, 128
    qkv_c, dout_c = R.make_inputs("random", B, N, H, kind, seed=1000 + N)
    qkv, dout = qkv_c.cuda(), dout_c.cuda()
    o, lse = _fwd(qkv, B, N, H, kind)
    d1 = _bwd(qkv, o, dout, lse, B, N, H, kind)
    d2 = _bwd(qkv, o, dout, lse, B, N, H, kind, vfirst=True)
    assert _same(d2[:, :D], d1[:, :D]) and _same(d2[:, D:2 * D], d1[:, 2 * D:]) and _same(d2[:, 2 * D:], d1[:, D:2 * D])
    d3 = _bwd(qkv, o, dout, lse, B, N, H, kind, vfirst=True, need_dk=False)
    assert _same(d3[:, :2 * D], d2[:, :2 * D])
    d4 = _bwd(qkv, o, dout, lse, B, N, H, kind, need_dk=False)
    assert _same(d4[:, :D], d1[:, :D]) and _same(d4[:, 2 * D:], d1[:, 2 * D:])


@pytest.mark.parametrize("N", [3, 17, 65])
def test_fp16_gradients_scale_with_a_power_of_two(N):
    """fp16 (the tf32h engine hands dout over times a power of two): dout 2^8 gives dqkv 2^8.  Every fp32 operation of the backward commutes with a
    power of two, and so does every fp16 rounding of a value that is a NORMAL fp16 number at both scales.  Asserted: bit equality of every gradient
    element that is a normal fp16 number at the lower scale; an element that is subnormal there (|x| < 2^-14: it keeps fewer bits than its scaled
    twin) agrees to half the subnormal spacing, 2^-25."""
    B, H, k = 2, 2, 8
    qkv_c, dout_c = R.make_inputs("random", B, N, H, "f16", seed=2000 + N)
    qkv, dout = qkv_c.cuda(), dout_c.cuda()
    big = dout * 2.0 ** k
    assert bool(torch.isfinite(big).all()) and torch.equal(big.float(), dout.float() * 2.0 ** k)
    o, lse = _fwd(qkv, B, N, H, "f16")
    d1 = _bwd(qkv, o, dout, lse, B, N, H, "f16").float()
    d2 = _bwd(qkv, o, big, lse, B, N, H, "f16").float() * 2.0 ** -k
    normal = d1.abs() >= 2.0 ** -14
    assert bool(torch.isfinite(d2).all()) and float(normal.float().mean()) > 0.99
    assert torch.equal(d1[normal], d2[normal]), f"{int((d1[normal] != d2[normal]).sum())} normal elements differ"
    assert float((d1 - d2)[~normal].abs().max() if bool((~normal).any()) else 0.0) <= 2.0 ** -25


# ------------------------------------------------------------------------------------------------ surroundings
GUARD = 4096          # bytes of canary before and after every view


def _guarded(nelem, dtype, fill=float("nan")):
    """-> (buffer, view of nelem elements with GUARD bytes of NaN canary on either side, the buffer's bits before the call)"""
    ge = GUARD // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((ge + nelem + ge,), float("nan"), dtype=dtype, device="cuda")
    view = buf[ge:ge + nelem]
    view.fill_(fill)
    return buf, view, ge


def _canaries_intact(buf, ge, nelem):
    nan_bits = _bits(torch.full((1,), float("nan"), dtype=buf.dtype, device="cuda"))[0]
    b = _bits(buf)
    return bool((b[:ge] == nan_bits).all()) and bool((b[ge + nelem:] == nan_bits).all())


def _padded_input(t, extra_rows):
    """t [rows, cols] followed by NaN rows inside one allocation -> the view of the first `rows` rows"""
    buf = torch.full((t.shape[0] + extra_rows, t.shape[1]), float("nan"), dtype=t.dtype, device="cuda")
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


SURROUND = [(kd, None, None) for kd in KINDS] + [(kd, "attn_dkv_nw", 4) for kd in SIXTEEN] + [(kd, "attn_dkv_nw", 8) for kd in SIXTEEN] + \
    [(kd, "attn_dkv_dma", 0) for kd in SIXTEEN]


@pytest.mark.parametrize("N", [1, 65, 129, 193, 257])
@pytest.mark.parametrize("kind,opt,val", SURROUND, ids=[f"{kd}-{(o or 'default')}{'' if v is None else v}" for kd, o, v in SURROUND])
def test_surroundings(kind, opt, val, N):
    """gd_attention_fwd / gd_attention_bwd on views of larger buffers.  Outputs and the workspace sit between NaN canaries that must come back
    bit-unchanged; the workspace is exactly gd_attention_bwd_workspace_bytes long and NaN-filled, and the gradients equal those of a zero-filled
    one (the dK/dV kernel reads only what the dQ kernel wrote, pad rows included); qkv, o, dout and lse are followed by NaN rows, and the results
    are finite and bit-identical to the plain run (the clamp to row N - 1 and the tail mask hide everything past N).  Every buffer is
    over-allocated: a stray access lands in a canary."""
    from gd_amd._lib import check, dtype_code, lib, ptr, stream
    from gd_amd.ops import F32X3
    for B, H in ((1, 1), (2, 2)):
        tag = f"{kind} {opt}={val} B={B} N={N} H={H}"
        qkv_c, dout_c = R.make_inputs("pair", B, N, H, kind, seed=3000 + N)
        qkv, dout = qkv_c.cuda(), dout_c.cuda()
        code = F32X3 if kind == "x3" else dtype_code(qkv)
        with _option(opt, val):
            o0, lse0 = _fwd(qkv, B, N, H, kind)
            g0 = _bwd(qkv, o0, dout, lse0, B, N, H, kind)
            # forward
            qkv_p = _padded_input(qkv, 70)
            obuf, o, oge = _guarded(B * N * H * 64, qkv.dtype)
            lbuf, lse, lge = _guarded(B * H * N, torch.float32)
            check(lib().gd_attention_fwd(ptr(qkv_p), ptr(o), ptr(lse), B, N, H, 64, 0.125, code, stream()), "gd_attention_fwd")
            assert _canaries_intact(obuf, oge, o.numel()) and _canaries_intact(lbuf, lge, lse.numel()), tag + ": forward wrote outside o / lse"
            assert _same(o, o0.view(-1)) and _same(lse, lse0.view(-1)), tag + ": forward changed by what follows qkv"
            # backward: NaN-filled workspace of exactly the stated size, then a zero-filled one
            nbytes = lib().gd_attention_bwd_workspace_bytes(B, N, H)
            assert nbytes == 2 * B * H * ((N + 63) // 64 * 64) * 4
            o_p, dout_p = _padded_input(o0, 70), _padded_input(dout, 70)
            lse_p = _padded_input(lse0.view(1, -1), 1).view(-1)            # as many NaN floats behind lse as lse is long
            outs = []
            for fill in (float("nan"), 0.0):
                gbuf, g, gge = _guarded(B * N * 3 * H * 64, qkv.dtype)
                wbuf, ws, wge = _guarded(nbytes // 4, torch.float32, fill)
                check(lib().gd_attention_bwd(ptr(qkv_p), ptr(o_p), ptr(dout_p), ptr(lse_p), ptr(g), ptr(ws), B, N, H, 64, 0.125, code, 0, stream()),
                      "gd_attention_bwd")
                assert _canaries_intact(gbuf, gge, g.numel()) and _canaries_intact(wbuf, wge, ws.numel()), tag + ": backward wrote outside dqkv / workspace"
                assert bool(torch.isfinite(g.float()).all()) and bool(torch.isfinite(ws).all()), tag + ": dqkv or the workspace not fully written"
                outs.append(g)
            assert _same(outs[0], outs[1]), tag + ": the gradients depend on what the workspace held"
            assert _same(outs[0], g0.view(-1)), tag + ": backward changed by what follows its inputs"
