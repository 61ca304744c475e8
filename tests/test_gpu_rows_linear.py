"""GPU: gd_rows_linear (csrc/rows.hip) per element against the fp64 restatement and its derived bound (tests/rows_ref64.py: the case table, the
input families and the bound are shared with tests/test_rows_ref_host.py, which shows on the CPU that each mutant breaks the bound), on operands that
sit inside wider NaN-filled buffers — the padding of every row stride and the rows around y must come back untouched, the inputs bit-identical — and
the bit equalities the kernel's fixed summation order promises: a row of an M-row call against the one-row call, a column block against the full-N
call, run to run, in place against out of place.  With GD_CAMERA_ERRORS=<file> the worst err / bound of every case is appended there
(profiles/camera_head_errors.txt)."""
import functools
import os

import pytest
import torch

import rows_ref64 as R

pytestmark = pytest.mark.gpu

IDS = [f"{i}-M{c['M']}-K{c['K']}-N{c['N']}-{c['wt']}" for i, c in enumerate(R.LINEAR_CASES)]
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GD_CAMERA_ERRORS")
    if path and _WORST:
        with open(path, "a") as f:
            f.write("# gd_rows_linear: worst err / bound per case (tests/test_gpu_rows_linear.py)\n")
            for k in sorted(_WORST):
                f.write(f"{_WORST[k]:8.4f}  rows_linear[{k}]\n")


@functools.lru_cache(maxsize=None)
def reference(i):
    """(host inputs, fp64 result, bound) of case i: computed once, shared, never modified."""
    c = R.LINEAR_CASES[i]
    inp = R.linear_inputs(c)
    want, bound = R.linear64(inp["x"], inp["w"], inp["bias"], inp["residual"], inp["gamma"], c["silu"], c["gelu"])
    return inp, want, bound


def padded(t, pad, rows_around=0):
    """t [R, C] on the device inside a NaN-filled buffer [R + 2 rows_around, C + pad] -> (buffer, view)."""
    R_, C = t.shape
    buf = torch.full((R_ + 2 * rows_around, C + pad), float("nan"), dtype=t.dtype, device="cuda")
    view = buf[rows_around:rows_around + R_, :C]
    view.copy_(t)
    return buf, view


def bits(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def run(c, inp, rows=None, cols=None, inplace=False):
    """The kernel on case c's operands (rows / cols: a slice of the rows of x or of the columns of w) -> y [M', N'] on the host; checks the canaries and
    that no input changed."""
    from gd_amd import ops
    rs, cs = rows if rows is not None else slice(None), cols if cols is not None else slice(None)
    px, pw, py = c["pads"]
    xbuf, x = padded(inp["x"][rs], px)
    wbuf, w = padded(inp["w"][cs], pw)
    dev = lambda t, *ix: None if t is None else t[ix].contiguous().cuda()
    bias, gamma = dev(inp["bias"], cs), dev(inp["gamma"], cs)
    M, N = x.shape[0], w.shape[0]
    py = py + (-(N + py)) % 4
    ybuf, y = padded(torch.zeros(M, N), py, rows_around=1)
    y.fill_(float("nan"))
    res = None
    if inp["residual"] is not None:
        r = inp["residual"][rs][:, cs]
        if inplace:
            y.copy_(r)
            res = y
        else:
            rbuf, res = padded(r, 4 + (-(N + 4)) % 4)
    before = [(t, bits(t).clone()) for t in (xbuf, wbuf, bias, gamma) + ((rbuf,) if res is not None and not inplace else ()) if t is not None]
    out = ops.rows_linear(x, w, bias, out=y, residual=res, gamma=gamma, silu=c["silu"], gelu=c["gelu"])
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    for t, b in before:
        assert torch.equal(bits(t), b), "an input changed"
    mask = torch.ones_like(ybuf, dtype=torch.bool)
    mask[1:1 + M, :N] = False
    assert bool(torch.isnan(ybuf[mask]).all()), "a cell outside y was written"
    return y.cpu().clone()


@pytest.mark.parametrize("i", range(len(R.LINEAR_CASES)), ids=IDS)
def test_rows_linear_per_element_against_fp64(i):
    c = R.LINEAR_CASES[i]
    inp, want, bound = reference(i)
    got = run(c, inp)
    assert got.dtype == torch.float32 and got.shape == want.shape and bool(torch.isfinite(got).all())
    ratio = (got.double() - want).abs() / bound
    worst = float(ratio.max())
    _WORST[IDS[i]] = worst
    print(f"rows_linear {IDS[i]} silu={c['silu']} gelu={c['gelu']} residual={c['residual']} gamma={c['gamma']}: worst err / bound {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("i", [5, 8, 11, 3], ids=lambda i: IDS[i])
def test_a_row_is_bit_identical_to_the_one_row_call(i):
    c = R.LINEAR_CASES[i]
    inp, _, _ = reference(i)
    full = run(c, inp)
    for m in (0, c["M"] - 1):
        one = run(c, inp, rows=slice(m, m + 1))
        assert torch.equal(bits(one[0]), bits(full[m])), m
    if c["M"] == 8:                                                            # and a 3-row call: another template instantiation
        three = run(c, inp, rows=slice(2, 5))
        assert torch.equal(bits(three), bits(full[2:5]))


@pytest.mark.parametrize("i", [6, 15, 2], ids=lambda i: IDS[i])
def test_a_column_block_is_bit_identical_to_the_full_call(i):
    """Another N, another grid, and columns that sit elsewhere in their wave and workgroup (the block starts at an odd column)."""
    c = R.LINEAR_CASES[i]
    inp, _, _ = reference(i)
    full = run(c, inp)
    for lo, hi in ((3, min(c["N"], 20)), (c["N"] - 1, c["N"]), (0, 1)):
        part = run(c, inp, cols=slice(lo, hi))
        assert torch.equal(bits(part), bits(full[:, lo:hi])), (lo, hi)


@pytest.mark.parametrize("i", [6, 12, 9], ids=lambda i: IDS[i])
def test_run_to_run_and_in_place_are_bit_identical(i):
    c = R.LINEAR_CASES[i]
    inp, _, _ = reference(i)
    first = run(c, inp)
    assert torch.equal(bits(run(c, inp)), bits(first))
    if c["residual"]:
        assert torch.equal(bits(run(c, inp, inplace=True)), bits(first))


def test_bf16_weights_are_held_to_the_fp32_bound_on_the_rounded_weights():
    """The restatement of a bf16 case IS fp64 on the bf16-rounded weights under the same bound: nothing in it knows the weight type but the chunk a
    mutant drops.  Against the unrounded weights the result is 2^-9 away — three orders of magnitude beyond the bound."""
    i = 15
    c = R.LINEAR_CASES[i]
    inp, want, bound = reference(i)
    again, _ = R.linear64(inp["x"], inp["w"].float(), inp["bias"], None, None, c["silu"], c["gelu"])
    assert torch.equal(again, want) and inp["w"].dtype == torch.bfloat16
