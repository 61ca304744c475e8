"""GPU: gd_tokens_linear (csrc/tokens_linear.hip) per element against the fp64 restatement and its derived bound (tests/tokens_linear_ref64.py: the
case table, the input families and the bound are shared with tests/test_tokens_linear_ref_host.py, which shows on the CPU that each mutant breaks the
bound), on operands that sit inside wider NaN-filled buffers — the padding of every row stride and the rows around y must come back untouched, the
inputs bit-identical — and the bit equalities the kernel's fixed summation order promises: a row block of an M-row call against the call on those rows
alone, a column block against the full-N call, run to run, in place against out of place.  One comparison with ops.gemm_nt under the same bound.
With GD_TOKENS_ERRORS=<file> the worst err / bound of every case is appended there (profiles/tokens_linear_errors.txt)."""
import functools
import os

import pytest
import torch

import tokens_linear_ref64 as R

pytestmark = pytest.mark.gpu
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GD_TOKENS_ERRORS")
    if path and _WORST:
        with open(path, "a") as f:
            f.write("# gd_tokens_linear: worst err / bound per case (tests/test_gpu_tokens_linear.py)\n")
            for k in sorted(_WORST):
                f.write(f"{_WORST[k]:8.4f}  tokens_linear[{k}]\n")


@functools.lru_cache(maxsize=None)
def reference(i):
    """(host inputs, fp64 result, bound) of case i: computed once, shared, never modified."""
    c = R.CASES[i]
    inp = R.inputs(c)
    want, bound = R.linear64(inp["x"], inp["w"], inp["bias"], inp["residual"], inp["y0"], c["gelu"], c["accumulate"])
    return inp, want, bound


def padded(t, pad, rows_around=0):
    """t [R, C] on the device inside a NaN-filled buffer [R + 2 rows_around, C + pad] -> (buffer, view)."""
    R_, C = t.shape
    buf = torch.full((R_ + 2 * rows_around, C + pad), float("nan"), dtype=t.dtype, device="cuda")
    view = buf[rows_around:rows_around + R_, :C]
    view.copy_(t)
    return buf, view


def bits(t):
    return t.view(torch.int32)


def run(c, inp, rows=None, cols=None, inplace=False):
    """The kernel on case c's operands (rows / cols: a slice of the rows of x or of the columns of w) -> y [M', N'] on the host; checks the canaries and
    that no input changed."""
    from gd_amd import ops
    rs, cs = rows if rows is not None else slice(None), cols if cols is not None else slice(None)
    px, pw, py = c["pads"]
    xbuf, x = padded(inp["x"][rs], px)
    wbuf, w = padded(inp["w"][cs], pw)
    bias = None if inp["bias"] is None else inp["bias"][cs].contiguous().cuda()
    M, N = x.shape[0], w.shape[0]
    py = py + (-(N + py)) % 4
    ybuf, y = padded(torch.zeros(M, N), py, rows_around=1)
    y.fill_(float("nan"))
    if c["accumulate"]:
        y.copy_(inp["y0"][rs][:, cs])
    res = rbuf = None
    if inp["residual"] is not None:
        r = inp["residual"][rs][:, cs]
        if inplace:
            assert not c["accumulate"]
            y.copy_(r)
            res = y
        else:
            rbuf, res = padded(r, 4 + (-(N + 4)) % 4)
    before = [(t, bits(t).clone()) for t in (xbuf, wbuf, bias, rbuf) if t is not None]
    out = ops.tokens_linear(x, w, bias, out=y, residual=res, gelu=c["gelu"], accumulate=c["accumulate"])
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    for t, b in before:
        assert torch.equal(bits(t), b), "an input changed"
    mask = torch.ones_like(ybuf, dtype=torch.bool)
    mask[1:1 + M, :N] = False
    assert bool(torch.isnan(ybuf[mask]).all()), "a cell outside y was written"
    return y.cpu().clone()


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=R.IDS)
def test_per_element_against_fp64(i):
    c = R.CASES[i]
    inp, want, bound = reference(i)
    got = run(c, inp)
    assert got.dtype == torch.float32 and got.shape == want.shape and bool(torch.isfinite(got).all())
    worst = float(((got.double() - want).abs() / bound).max())
    _WORST[R.IDS[i]] = worst
    print(f"tokens_linear {R.IDS[i]} bias={c['bias']} gelu={c['gelu']} residual={c['residual']} accumulate={c['accumulate']} tall tiles={R.tall_tiles(c)}: "
          f"worst err / bound {worst:.4f}")
    assert worst <= 1.0


def test_allocated_output_has_rows_padded_to_a_multiple_of_four():
    from gd_amd import ops
    from gd_amd._lib import GdHipError
    i = 6
    c = R.CASES[i]
    inp, want, bound = reference(i)
    x, w, b = inp["x"].cuda(), inp["w"].cuda(), inp["bias"].cuda()
    y = ops.tokens_linear(x, w, b)
    assert tuple(y.shape) == (c["M"], c["N"]) and y.stride() == (c["N"] + (-c["N"]) % 4, 1)
    assert float(((y.cpu().double() - want).abs() / bound).max()) <= 1.0
    with pytest.raises(GdHipError, match="accumulate"):
        ops.tokens_linear(x, w, b, accumulate=True)


@pytest.mark.parametrize("i", [5, 6, 9, 11], ids=lambda i: R.IDS[i])
def test_a_row_block_is_bit_identical_to_the_call_on_those_rows(i):
    """Rows 0 and M - 1 alone and an interior block that starts inside a tile: another M, another grid, other places in the tiles — and for the last
    case the other tile height (the full call runs on 64 x 32 tiles, the blocks on 32 x 32)."""
    c = R.CASES[i]
    inp, _, _ = reference(i)
    full = run(c, inp)
    M = c["M"]
    blocks = [(0, 1), (M - 1, M), (5, min(M - 1, 5 + 40))]
    for lo, hi in blocks:
        part = run(c, inp, rows=slice(lo, hi))
        assert torch.equal(bits(part), bits(full[lo:hi])), (lo, hi)
    if i == 11:
        assert R.tall_tiles(c) and not R.tall_tiles(dict(c, M=40))


@pytest.mark.parametrize("i", [6, 8, 4], ids=lambda i: R.IDS[i])
def test_a_column_block_is_bit_identical_to_the_full_call(i):
    """Another N, another grid, and columns that sit elsewhere in their tile (the block starts at column 3)."""
    c = R.CASES[i]
    inp, _, _ = reference(i)
    full = run(c, inp)
    for lo, hi in ((3, min(c["N"], 20)), (c["N"] - 1, c["N"]), (0, 1)):
        part = run(c, inp, cols=slice(lo, hi))
        assert torch.equal(bits(part), bits(full[:, lo:hi])), (lo, hi)


@pytest.mark.parametrize("i", [9, 8, 6, 11], ids=lambda i: R.IDS[i])
def test_run_to_run_and_in_place_are_bit_identical(i):
    c = R.CASES[i]
    inp, _, _ = reference(i)
    first = run(c, inp)
    assert torch.equal(bits(run(c, inp)), bits(first))
    if c["residual"] and not c["accumulate"]:
        assert torch.equal(bits(run(c, inp, inplace=True)), bits(first))


def test_gemm_nt_on_the_same_operands_lies_inside_the_same_bound():
    """Both kernels are held to the fp64 bound of the case; they need not be equal (gd_gemm_nt sums k in one chain, this kernel in four)."""
    from gd_amd import ops
    i = 9
    c = R.CASES[i]
    inp, want, bound = reference(i)
    x, w, b, r = (inp[k].cuda() for k in ("x", "w", "bias", "residual"))
    ours = ops.tokens_linear(x, w, b, residual=r, gelu=True)
    theirs = ops.gemm_nt(x, w, bias=b, act=1, residual=r)
    e = [float(((t.cpu().double() - want).abs() / bound).max()) for t in (ours, theirs)]
    differ = int((bits(ours) != bits(theirs)).sum())
    print(f"tokens_linear vs gemm_nt at {R.IDS[i]}: worst err / bound {e[0]:.4f} and {e[1]:.4f}; {differ} of {ours.numel()} elements differ in their bits")
    assert e[0] <= 1.0 and e[1] <= 1.0
