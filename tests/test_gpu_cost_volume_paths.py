"""Cost-volume KL (csrc/cost_volume.hip) PER ROW and PER ELEMENT against the fp64 restatement of tests/cv_ref64.py, on every dispatch path, at the C ABI:
|got - ref64| <= bound(element) for tstats, the four stats fields, loss, df1 and df2 separately, the bounds derived there from the kernels' operation
order, never measured.  Three input families (random with cosines over [-0.9, 0.9], norms over decades, clamped / zero rows; the exact-score probe whose
scores are exactly -1 / 0 / 1 in every operand type; the selector probe that keeps one row per (pair, view) at a tile edge): tests/test_cv_ref_host.py shows
that every mutant of the restatement violates these bounds by a factor >= 4.  Every workspace is NaN-filled and exactly ..._workspace_bytes long, every
output is an interior slice of a NaN-filled allocation whose guards must come back bit-unchanged, the inputs (teacher pad columns included) are compared
bit for bit afterwards, two runs are bit-identical, a zero loss gradient gives exactly zero gradients, and no NaN leaves a kernel.
With GD_CV_ERRORS=<file> the worst err / bound of every (path, kind, family, output) group is written there (profiles/cost_volume_errors.txt).

CASES is the path table; `expected_kernel` restates the dispatch predicate of cv_fwd_common / cv_bwd_tiles_launch and every case asserts the kernel it is
meant to reach (profiles/cost_volume_path_coverage.txt records what a kernel trace saw).  Sizes: every case runs the two probes at every hw of GRID with
P = 3 (the odd-ldt case at the sizes that are no multiple of 4) and the random family at RANDOM_HW.  P = 1 is covered by
test_pair_alone_equals_pair_in_batch."""
import os

import pytest
import torch

import cv_ref64 as R

pytestmark = pytest.mark.gpu

GRID = [1, 5, 63, 64, 65, 127, 128, 129, 191, 257, 385]
RANDOM_HW = [5, 65, 129, 385]
ODD = [h for h in GRID if h % 4]
OPTION_DEFAULTS = {"cv_persist": 1, "cv_mask_skip": 1, "cv_grid": 0}
_WORST = {}


def expected_kernel(kind, C, ldt, t_aligned16, persist=1):
    """cv_fwd_common / cv_bwd_tiles_launch: the persistent kernel (forward, and its BWD instantiation) or the tile kernel with one of its two main loops"""
    rowb = C * (4 if kind == "f32" else 2)
    if persist and rowb % 128 == 0 and rowb >= 384 and ldt % 4 == 0 and t_aligned16:
        return "persist"
    return "tile/dma_mainloop" if rowb % 128 == 0 else "tile/mma_tile_128x128"


def _case(name, kind, C, path, sizes, ldt=4, toff=0, prenorm=False, given_tstats=True, **opts):
    return dict(name=name, kind=kind, C=C, path=path, sizes=sizes, ldt=ldt, toff=toff, prenorm=prenorm or kind == "f16", given_tstats=given_tstats, opts=opts)


# ldt: 4 / 32 = hw rounded up to that many floats, 0 = hw itself; toff: teacher pointer offset in floats; prenorm: ..._fwd_prenorm (cv_stats_init_kernel)
# instead of ..._fwd (cv_norm_kernel); given_tstats False: tstats null (the forward runs cv_tstats_kernel into its workspace)
CASES = [
    _case("mma-f32-C20", "f32", 20, "tile/mma_tile_128x128", GRID, given_tstats=False),
    _case("mma-f32-C4", "f32", 4, "tile/mma_tile_128x128", GRID, prenorm=True),
    _case("mma-f32-C80", "f32", 80, "tile/mma_tile_128x128", GRID, ldt=0),
    _case("mma-bf16-C40", "bf16", 40, "tile/mma_tile_128x128", GRID, prenorm=True),
    _case("mma-bf16-C8", "bf16", 8, "tile/mma_tile_128x128", GRID, given_tstats=False, ldt=0),
    _case("mma-bf16-C200", "bf16", 200, "tile/mma_tile_128x128", GRID),
    _case("dma1-f32-C32", "f32", 32, "tile/dma_mainloop", GRID, prenorm=True, given_tstats=False),
    _case("dma2-f32-C64", "f32", 64, "tile/dma_mainloop", GRID),
    _case("dma1-bf16-C64", "bf16", 64, "tile/dma_mainloop", GRID, given_tstats=False),
    _case("dma2-bf16-C128", "bf16", 128, "tile/dma_mainloop", GRID),
    _case("dma1-f16-C64", "f16", 64, "tile/dma_mainloop", GRID),
    _case("dma2-f16-C128", "f16", 128, "tile/dma_mainloop", GRID, given_tstats=False),
    _case("oddldt-f32-C96", "f32", 96, "tile/dma_mainloop", ODD, ldt=0),
    _case("nopersist-f32-C96", "f32", 96, "tile/dma_mainloop", GRID, cv_persist=0),
    _case("nopersist-bf16-C192", "bf16", 192, "tile/dma_mainloop", GRID, cv_persist=0, prenorm=True),
    _case("nopersist-f16-C192", "f16", 192, "tile/dma_mainloop", GRID, cv_persist=0),
    _case("toff-f32-C96", "f32", 96, "tile/dma_mainloop", GRID, toff=1),
    _case("persist-f32-C96", "f32", 96, "persist", GRID, cv_grid=8),
    _case("persist-f32-C160", "f32", 160, "persist", GRID, cv_grid=8, prenorm=True, given_tstats=False),
    _case("persist-bf16-C192", "bf16", 192, "persist", GRID, cv_grid=8, prenorm=True),
    _case("persist-bf16-C320", "bf16", 320, "persist", GRID, cv_grid=8, ldt=32),
    _case("persist-f16-C192", "f16", 192, "persist", GRID, cv_grid=8),
    _case("persist-noskip-f32-C96", "f32", 96, "persist", GRID, cv_grid=8, cv_mask_skip=0),
    _case("persist-noskip-bf16-C192", "bf16", 192, "persist", GRID, cv_grid=8, cv_mask_skip=0, ldt=32),
    _case("persist-fullgrid-f32-C96", "f32", 96, "persist", [385], ldt=32),
]
DENSE = [(c, hw) for c in CASES for hw in c["sizes"]]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GD_CV_ERRORS")
    if path and _WORST:
        with open(path, "w") as f:
            for k in sorted(_WORST):
                f.write(f"{_WORST[k][0]:8.4f}  {k:52s} worst at {_WORST[k][1]}\n")


class _options:
    """Library options off their defaults for the duration of a `with` block."""

    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        from gd_amd._lib import check, lib
        for name, value in self.opts.items():
            assert lib().gd_debug_get(name.encode()) == OPTION_DEFAULTS[name], f"{name} is not at its default"
            check(lib().gd_debug_set(name.encode(), value), "gd_debug_set")

    def __exit__(self, *exc):
        from gd_amd._lib import lib
        for name in self.opts:
            lib().gd_debug_set(name.encode(), OPTION_DEFAULTS[name])
            assert lib().gd_debug_get(name.encode()) == OPTION_DEFAULTS[name]


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


GUARD = 4096          # bytes of canary before and after every view


class _Guarded:
    """A NaN-filled (all bits set) allocation and the interior view a kernel writes."""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((GUARD + self.nbytes + GUARD,), 0xFF, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.nbytes].view(dtype).view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == 0xFF).all()) and bool((self.buf[GUARD + self.nbytes:] == 0xFF).all())


def _workspace(nbytes):
    return _Guarded((nbytes,), torch.uint8)


def _check(group, what, got, ref, bound, tag):
    worst, idx = R.ratio(got.cpu(), ref, bound)
    key = f"{group} {what}"
    if worst > _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (worst, f"{tag} index {idx}")
    assert worst <= 1.0, (f"{group} / {what} / {tag}: worst err / bound = {worst:.3f} at {idx}: got {float(got[idx])!r}, ref {float(ref[idx])!r}, "
                          f"bound {float(bound[idx]):.3e}")


class _Device:
    """One Inputs on the GPU in a case's layout: operands, masters, fp32 inverse norms, teacher maps [P, hw, ldt] with zero pads (optionally offset by
    `toff` floats from a 16-byte boundary), masks, loss gradients — and their bits, to show afterwards that nothing was written to."""

    def __init__(self, x, ldt_mode, toff):
        hw, P = x.hw, x.P
        self.x = x
        self.ldt = hw if ldt_mode == 0 else (hw + ldt_mode - 1) // ldt_mode * ldt_mode
        a, b = x.operands()
        self.fa, self.fb = a.cuda().contiguous(), b.cuda().contiguous()
        self.f1m, self.f2m = x.f1.cuda().contiguous(), x.f2.cuda().contiguous()
        self.inv = tuple(t.cuda() for t in x.inv32())
        self.t = []
        for T in (x.t1, x.t2):
            buf = torch.zeros(P * hw * self.ldt + 4, dtype=torch.float32, device="cuda")
            v = buf[toff:toff + P * hw * self.ldt].view(P, hw, self.ldt)
            v[:, :, :hw] = T.cuda()
            assert v.data_ptr() % 16 == 4 * toff
            self.t.append(v)
        self.m = (x.m1.to(torch.uint8).cuda(), x.m2.to(torch.uint8).cuda())
        self.gloss = x.gloss.cuda()
        self.inputs = [self.fa, self.fb, self.f1m, self.f2m, *self.inv, *self.t, *self.m, self.gloss]
        self.before = [_bits(t).clone() for t in self.inputs]

    def unchanged(self):
        return all(torch.equal(_bits(t), b) for t, b in zip(self.inputs, self.before)) and \
            all(float(t[:, :, self.x.hw:].abs().max()) == 0.0 for t in self.t if self.ldt > self.x.hw)


def _tstats(dev):
    from gd_amd._lib import check, lib, ptr, stream
    x = dev.x
    out = _Guarded((x.P, 2, x.hw, 4), torch.float32)
    check(lib().gd_cost_volume_teacher_stats(ptr(dev.t[0]), ptr(dev.t[1]), x.P, x.hw, dev.ldt, ptr(out.view), stream()), "gd_cost_volume_teacher_stats")
    assert out.intact(), "teacher_stats wrote outside tstats"
    return out.view


def _forward(dev, variant, tstats, prenorm, kcap=0):
    """-> (loss [P], stats [P, 2, hw, 4]) through gd_cost_volume_kl_fwd / _fwd_prenorm / _fwd_rows (kcap > 0) on guarded buffers and a NaN workspace"""
    from gd_amd._lib import check, lib, ptr, stream
    x = dev.x
    P, hw, C = x.P, x.hw, x.C
    code, vi = R.KINDS[x.kind][1], R.VARIANTS.index(variant)
    loss, stats = _Guarded((P,), torch.float32), _Guarded((P, 2, hw, 4), torch.float32)
    t1, t2, m1, m2 = dev.t[0], dev.t[1], dev.m[0], dev.m[1]
    if kcap:
        ws = _workspace(lib().gd_cost_volume_kl_rows_workspace_bytes(P, hw, kcap))
        rc = lib().gd_cost_volume_kl_fwd_rows(ptr(dev.fa), ptr(dev.fb), ptr(dev.inv[0]), ptr(dev.inv[1]), ptr(t1), ptr(t2), dev.ldt, ptr(tstats), ptr(m1), ptr(m2),
                                              P, hw, C, kcap, vi, code, ptr(loss.view), ptr(stats.view), ptr(ws.view), stream())
    else:
        ws = _workspace(lib().gd_cost_volume_kl_workspace_bytes(P, hw, C, code, 0))
        if prenorm:
            rc = lib().gd_cost_volume_kl_fwd_prenorm(ptr(dev.fa), ptr(dev.fb), ptr(dev.inv[0]), ptr(dev.inv[1]), ptr(t1), ptr(t2), dev.ldt, ptr(tstats), ptr(m1),
                                                     ptr(m2), P, hw, C, vi, code, ptr(loss.view), ptr(stats.view), ptr(ws.view), stream())
        else:
            rc = lib().gd_cost_volume_kl_fwd(ptr(dev.fa), ptr(dev.fb), ptr(t1), ptr(t2), dev.ldt, ptr(tstats), ptr(m1), ptr(m2), P, hw, C, vi, code,
                                             ptr(loss.view), ptr(stats.view), ptr(ws.view), stream())
    check(rc, "gd_cost_volume_kl_fwd*")
    torch.cuda.synchronize()
    assert loss.intact() and stats.intact() and ws.intact(), "the forward wrote outside loss / stats / its workspace"
    return loss.view, stats.view


def _backward(dev, stats, kcap=0):
    """-> (df1, df2) through gd_cost_volume_kl_bwd / _bwd_h / _bwd_rows (kcap > 0)"""
    from gd_amd._lib import check, lib, ptr, stream
    x = dev.x
    P, hw, C = x.P, x.hw, x.C
    code = R.KINDS[x.kind][1]
    h = x.kind == "f16"
    gdt = torch.float32 if h else dev.fa.dtype
    df1, df2 = _Guarded((P, hw, C), gdt), _Guarded((P, hw, C), gdt)
    t1, t2, m1, m2 = dev.t[0], dev.t[1], dev.m[0], dev.m[1]
    if kcap:
        ws = _workspace(lib().gd_cost_volume_kl_bwd_rows_workspace_bytes(P, hw, C, kcap, code))
        f1, f2 = (dev.f1m, dev.f2m) if h else (dev.fa, dev.fb)
        rc = lib().gd_cost_volume_kl_bwd_rows(ptr(f1), ptr(f2), ptr(dev.fa) if h else None, ptr(dev.fb) if h else None, ptr(t1), ptr(t2), dev.ldt, ptr(m1), ptr(m2),
                                              P, hw, C, kcap, code, ptr(dev.gloss), ptr(stats), ptr(df1.view), ptr(df2.view), ptr(ws.view), stream())
    elif h:
        ws = _workspace(lib().gd_cost_volume_kl_bwd_h_workspace_bytes(P, hw, C))
        rc = lib().gd_cost_volume_kl_bwd_h(ptr(dev.f1m), ptr(dev.f2m), ptr(dev.fa), ptr(dev.fb), ptr(t1), ptr(t2), dev.ldt, ptr(m1), ptr(m2), P, hw, C,
                                           ptr(dev.gloss), ptr(stats), ptr(df1.view), ptr(df2.view), ptr(ws.view), stream())
    else:
        ws = _workspace(lib().gd_cost_volume_kl_workspace_bytes(P, hw, C, code, 1))
        rc = lib().gd_cost_volume_kl_bwd(ptr(dev.fa), ptr(dev.fb), ptr(t1), ptr(t2), dev.ldt, ptr(m1), ptr(m2), P, hw, C, code, ptr(dev.gloss), ptr(stats),
                                         ptr(df1.view), ptr(df2.view), ptr(ws.view), stream())
    check(rc, "gd_cost_volume_kl_bwd*")
    torch.cuda.synchronize()
    assert df1.intact() and df2.intact() and ws.intact(), "the backward wrote outside df1 / df2 / its workspace"
    return df1.view, df2.view


def _check_tstats(group, tag, x, ts):
    ref, bnd = R.teacher_stats64(x)
    for k, what in enumerate(("tstats.rowsum", "tstats.W", "tstats.A", "tstats.zero")):
        _check(group, what, ts[..., k], ref[..., k], bnd[..., k], tag)


def _check_forward(group, tag, x, variant, loss, stats, inv, ts, keep=None):
    """keep [P, 2, hw] bool: the rows whose logZ and W the path defines (None: all)"""
    ref = R.forward64(x, variant, inv=inv, tstats=ts)
    _check(group, "loss", loss, ref["loss"], ref["b_loss"], tag)
    for k, what in enumerate(("stats.inv", "stats.rowsum", "stats.logZ", "stats.W")):
        got, r, b = stats[..., k].cpu(), ref["stats"][..., k], ref["b_stats"][..., k]
        if keep is not None and k >= 2:
            got, r, b = got[keep], r[keep], b[keep]
        _check(group, what, got, r, b, tag)


def _check_backward(group, tag, x, stats, df1, df2, kcap=0):
    r1, r2, b1, b2 = R.backward64(x, stats.cpu(), kcap=kcap)
    _check(group, "df1", df1, r1, b1, tag)
    _check(group, "df2", df2, r2, b2, tag)
    zero = x.gloss == 0
    if bool(zero.any()):
        assert float(df1[zero.cuda()].float().abs().max()) == 0.0 and float(df2[zero.cuda()].float().abs().max()) == 0.0, f"{group} {tag}: zero loss gradient"


def _run_dense(case, hw, family, P=3):
    kind, C = case["kind"], case["C"]
    x = R.make_inputs(family, P, hw, C, kind)
    dev = _Device(x, case["ldt"], case["toff"])
    assert expected_kernel(kind, C, dev.ldt, case["toff"] == 0, case["opts"].get("cv_persist", 1)) == case["path"], \
        f"{case['name']} hw={hw}: the case table and the dispatch predicate disagree"
    group, tag = f"{case['name']} {family}", f"P={P} hw={hw}"
    ts = _tstats(dev)
    _check_tstats(group, tag, x, ts)
    given = ts if case["given_tstats"] else None
    inv = dev.inv if case["prenorm"] else None
    with _options(case["opts"]):
        outs = []
        for variant in R.VARIANTS:
            loss, stats = _forward(dev, variant, given, case["prenorm"])
            _check_forward(f"{group} {variant}", tag, x, variant, loss, stats, x.inv32() if inv else None, given.cpu() if given is not None else None)
            outs.append((loss, stats))
        assert _same(outs[0][1], outs[1][1]), f"{group} {tag}: stats depend on the variant"
        loss, stats = outs[1]
        df1, df2 = _backward(dev, stats)
        _check_backward(group, tag, x, stats, df1, df2)
        l2, s2 = _forward(dev, R.VARIANTS[1], given, case["prenorm"])
        g1, g2 = _backward(dev, s2)
        assert _same(loss, l2) and _same(stats, s2) and _same(df1, g1) and _same(df2, g2), f"{group} {tag}: two runs differ"
    assert dev.unchanged(), f"{group} {tag}: an input (or a teacher pad column) was written to"


@pytest.mark.parametrize("case,hw", DENSE, ids=[f"{c['name']}-{hw}" for c, hw in DENSE])
def test_dense_paths(case, hw):
    for family in R.FAMILIES:
        if family == "random" and hw not in RANDOM_HW:
            continue
        _run_dense(case, hw, family)


@pytest.mark.parametrize("hw", [1, 64, 65, 1536, 1537, 1600])
def test_teacher_stats_alone(hw):
    """cv_tstats_kernel by itself: 1536 = 64 * CV_TROW_MAX is the last size of the in-register form, 1537 and 1600 take the second pass over memory.
    Rows with a zero sum, a single entry and entries under the clamp; ldt = hw and ldt = hw rounded up to 4."""
    x = R.make_inputs("random", 1, hw, 4, "f32")
    for ldt_mode in (0, 4):
        dev = _Device(x, ldt_mode, 0)
        ts = _tstats(dev)
        _check_tstats(f"tstats ldt%{ldt_mode}", f"hw={hw}", x, ts)
        assert _same(ts, _tstats(dev)) and dev.unchanged()


def test_forward_hw1537():
    """One f32 forward past the in-register teacher row (hw = 1537, C = 32, P = 1), tstats null: cv_tstats_kernel's second pass inside the forward,
    13 x 13 tiles with a one-column ragged edge."""
    x = R.make_inputs("exact", 1, 1537, 32, "f32")
    dev = _Device(x, 0, 0)
    loss, stats = _forward(dev, "mast3r", None, False)
    _check_forward("dma1-f32-C32 exact mast3r", "P=1 hw=1537", x, "mast3r", loss, stats, None, None)
    assert dev.unchanged()


@pytest.mark.parametrize("name", ["mma-f32-C20", "dma2-bf16-C128", "dma1-f16-C64", "persist-f32-C96", "persist-bf16-C192", "persist-f16-C192"])
@pytest.mark.parametrize("hw", [129, 385])
def test_pair_alone_equals_pair_in_batch(name, hw):
    """Pair p computed alone (P = 1) is bit-identical to pair p of the batch of three: loss, stats, df1, df2.  Nothing in a tile's arithmetic depends on
    P: the tile kernels take the pair from blockIdx.y, the persistent kernels walk a pair-major tile list and reduce every row's slabs in a fixed order.
    The one exception: the fp16 G is stored under ONE power-of-two scale taken from the largest |dloss| of the batch (cv_gscale_kernel), so an fp16
    gradient is compared against the single pair's only for the pair that sets the scale; the others are held to their bounds by test_dense_paths."""
    case = next(c for c in CASES if c["name"] == name)
    x = R.make_inputs("exact", 3, hw, case["C"], case["kind"])
    dev = _Device(x, case["ldt"], 0)
    with _options(case["opts"]):
        ts = _tstats(dev)
        loss, stats = _forward(dev, "vggt", ts, case["prenorm"])
        df1, df2 = _backward(dev, stats)
        top = int(x.gloss.abs().argmax())
        for p in range(3):
            x1 = R.Inputs(x.f1[p:p + 1], x.f2[p:p + 1], x.t1[p:p + 1], x.t2[p:p + 1], x.m1[p:p + 1], x.m2[p:p + 1], x.gloss[p:p + 1], x.kind, x.family)
            d1 = _Device(x1, case["ldt"], 0)
            t1 = _tstats(d1)
            l1, s1 = _forward(d1, "vggt", t1, case["prenorm"])
            assert _same(t1[0], ts[p]) and _same(l1[0], loss[p]) and _same(s1[0], stats[p]), f"{name} hw={hw}: forward of pair {p}"
            if case["kind"] != "f16" or p == top:
                g1, g2 = _backward(d1, s1)
                assert _same(g1[0], df1[p]) and _same(g2[0], df2[p]), f"{name} hw={hw}: backward of pair {p}"


# ------------------------------------------------------------------------------------------------ kept-row form
ROWS = [(kind, C, hw, kcap) for kind, C in (("f32", 96), ("bf16", 192), ("f16", 192)) for hw, kcap in ((257, 128), (385, 128), (513, 128), (513, 256))]
KEPT_COUNTS = [0, 1, 127, 128, 128, 1]          # per (pair, view), P = 3


def _with_kept_counts(x, counts):
    """the masks of x replaced by masks with exactly counts[2 p + d] kept rows, the first and the last row among them where the count allows"""
    g = torch.Generator().manual_seed(x.hw)
    for p in range(x.P):
        for d, m in ((0, x.m1), (1, x.m2)):
            n = counts[2 * p + d]
            m[p] = False
            if n >= 1:
                m[p, x.hw - 1] = True
            if n >= 2:
                m[p, 0] = True
                rest = torch.randperm(x.hw - 2, generator=g)[:n - 2] + 1
                m[p, rest] = True
            assert int(m[p].sum()) == n
    return x


@pytest.mark.parametrize("kind,C,hw,kcap", ROWS)
def test_kept_row_paths(kind, C, hw, kcap):
    """gd_cost_volume_kl_fwd_rows / _bwd_rows (cv_rows_compact, cv_fwd_rows, cv_finalize_rows, cv_rows_gather, cv_bwd_rows, cv_rows_scatter) with 0, 1, 127 and
    128 kept rows per (pair, view), and the selector probe (one kept row at a tile edge).  logZ and W are compared at the kept rows' ORIGINAL indices; a
    masked row's logZ and W are NOT written by this path (the canary is still there) while inv and rowsum are.  Then the dense backward on the same
    stats (the option cv_bwd_rows = 0 of the wrapper): it selects by the mask and never reads a masked row's logZ / W."""
    for family in R.FAMILIES:
        x = R.make_inputs(family, 3, hw, C, kind)
        if family != "selector":
            x = _with_kept_counts(x, KEPT_COUNTS)
        dev = _Device(x, 4, 0)
        group, tag = f"rows{kcap}-{kind}-C{C} {family}", f"P=3 hw={hw}"
        keep = torch.stack([x.m1, x.m2], 1)
        with _options({"cv_grid": 8}):
            ts = _tstats(dev)
            outs = []
            for variant in R.VARIANTS:
                loss, stats = _forward(dev, variant, ts, True, kcap=kcap)
                _check_forward(f"{group} {variant}", tag, x, variant, loss, stats, x.inv32(), ts.cpu(), keep=keep)
                outs.append((loss, stats))
            loss, stats = outs[1]
            untouched = _bits(stats[..., 2:][~keep.cuda()])
            assert bool((untouched == 0xFF).all()), f"{group} {tag}: a masked row's logZ / W was written"
            df1, df2 = _backward(dev, stats, kcap=kcap)
            _check_backward(group, tag, x, stats, df1, df2, kcap=kcap)
            l2, s2 = _forward(dev, R.VARIANTS[1], ts, True, kcap=kcap)
            g1, g2 = _backward(dev, s2, kcap=kcap)
            assert _same(loss, l2) and _same(stats, s2) and _same(df1, g1) and _same(df2, g2), f"{group} {tag}: two runs differ"
            d1, d2 = _backward(dev, stats)
            _check_backward(f"{group} dense-bwd", tag, x, stats, d1, d2)
        assert dev.unchanged(), f"{group} {tag}: an input was written to"


def test_kept_rows_over_capacity_is_poisoned():
    """The one documented source of NaN: more kept rows than the capacity in one (pair, view).  That pair's loss is NaN and its gradients hold NaN —
    never a silently truncated sum; the other pairs are untouched: within their bounds, finite."""
    hw, C, kcap, bad = 385, 192, 128, 1
    x = _with_kept_counts(R.make_inputs("exact", 3, hw, C, "bf16"), [5, 128, 129, 7, 128, 1])
    dev = _Device(x, 4, 0)
    ts = _tstats(dev)
    loss, stats = _forward(dev, "vggt", ts, True, kcap=kcap)
    df1, df2 = _backward(dev, stats, kcap=kcap)
    ref = R.forward64(x, "vggt", inv=x.inv32(), tstats=ts.cpu())
    r1, r2, b1, b2 = R.backward64(x, stats.cpu(), kcap=kcap)
    assert bool(torch.isnan(loss[bad])) and bool(torch.isnan(df1[bad].float()).any())
    for p in (0, 2):
        _check("rows128-bf16-C192 over-capacity", "loss", loss[p:p + 1], ref["loss"][p:p + 1], ref["b_loss"][p:p + 1], f"pair {p}")
        _check("rows128-bf16-C192 over-capacity", "df1", df1[p], r1[p], b1[p], f"pair {p}")
        _check("rows128-bf16-C192 over-capacity", "df2", df2[p], r2[p], b2[p], f"pair {p}")


# ------------------------------------------------------------------------------------------------ the wrapper's routing
def _abi(x, variant, prenorm, given_tstats, kcap=0, ldt_mode=4):
    dev = _Device(x, ldt_mode, 0)
    ts = _tstats(dev)
    loss, stats = _forward(dev, variant, ts if given_tstats else None, prenorm, kcap=kcap)
    df1, df2 = _backward(dev, stats, kcap=kcap)
    return dev, ts, loss, df1, df2


@pytest.mark.parametrize("engine", ["f32", "bf16", "f32-inv", "h", "rows-bf16", "rows-h", "x3"])
def test_wrapper_routing(engine):
    """ops.cost_volume_kl once per engine: x3=False without and with inv_norms and tstats=None, x3="h", kept_rows_max (bf16 and "h"), held BIT-IDENTICAL
    in loss and gradients to the C ABI sequence the wrapper is meant to run (the one the tests above hold to the fp64 bounds); x3=True (the split bf16
    product, K = 3 C): the loss against the fp64 reference on the fp32 features with 2^-17 per operand on the score; its backward is the f32 dense
    backward the tests above bound, on stats the wrapper keeps to itself, so its gradients are only required to be finite here."""
    from gd_amd import ops
    kind = {"f32": "f32", "bf16": "bf16", "f32-inv": "f32", "h": "f16", "rows-bf16": "bf16", "rows-h": "f16", "x3": "f32"}[engine]
    hw, C, variant = 385, 192, "mast3r"
    x = R.make_inputs("random", 3, hw, C, kind)
    rows = engine.startswith("rows")
    if rows:
        x = _with_kept_counts(x, KEPT_COUNTS)
    prenorm, given = engine not in ("f32", "bf16"), engine not in ("f32", "f32-inv")
    dev, ts, loss, df1, df2 = _abi(x, variant, prenorm, given, kcap=128 if rows else 0)
    f1 = (dev.f1m if kind == "f16" else dev.fa).clone().requires_grad_(True)
    f2 = (dev.f2m if kind == "f16" else dev.fb).clone().requires_grad_(True)
    kw = {}
    if prenorm:
        kw["inv_norms"] = dev.inv
    if given:
        kw["tstats"] = ts
    if kind == "f16":
        kw["x3"], kw["h16"] = "h", (dev.fa, dev.fb)
    if engine == "x3":
        kw["x3"] = True
    if rows:
        kw["kept_rows_max"] = 128
    out = ops.cost_volume_kl(f1, f2, dev.t[0], dev.t[1], x.m1.cuda(), x.m2.cuda(), variant, **kw)
    (out * dev.gloss).sum().backward()
    if engine != "x3":
        assert _same(out.detach(), loss) and _same(f1.grad, df1) and _same(f2.grad, df2), f"{engine}: the wrapper and the C ABI sequence differ"
        return
    ref = R.forward64(x, variant, inv=x.inv32(), tstats=ts.cpu(), split_slack=R.U_X3)
    _check("wrapper x3", "loss", out.detach(), ref["loss"], ref["b_loss"], "P=3 hw=385")
    assert bool(torch.isfinite(f1.grad).all()) and bool(torch.isfinite(f2.grad).all())
