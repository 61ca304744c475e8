"""GPU: gd_attention_small_fwd (csrc/small_attn.hip, ops.attention_small_fwd) per element against the fp64 restatement and the bound of
tests/small_attn_ref64.py: |got - ref64| <= bound.  The shapes are the smallest at which the kernel can go wrong: one key, the 2 x 2 problems of the
time stage, head dimensions 4 / 12 / 48 / 64 (idle lanes in a 16-lane team, or none), Nk on both sides of the two kernels' threshold (8 | 9), ragged
last tiles, more keys than one pass of a wave covers, many short sequences with a ragged last wave.  Every worst ratio is printed before it is asserted."""
import functools

import pytest
import torch

import small_attn_ref64 as A64

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4, 1), (2, 2, 48, 8), (3, 3, 12, 8), (15, 17, 48, 2), (16, 16, 64, 1), (17, 65, 48, 8), (64, 300, 48, 8), (300, 64, 48, 8),
          (33, 129, 12, 3), (5, 8, 48, 2), (7, 9, 12, 3)]                    # (Nq, Nk, head_dim, H); the last two: the short / split threshold
GROUPS = [(1, 1), (3, 2), (41, 1)]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def worst(got, want, bound):
    ratio = (got.double() - want).abs() / bound.clamp_min(A64.TINY)
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), float((got.double() - want).abs().reshape(-1)[i]), float(bound.reshape(-1)[i])


@functools.lru_cache(maxsize=None)
def dense_case(Nq, Nk, hd, H, G0, G1, mag):
    g = gen(Nq * 1000 + Nk * 10 + hd + G0)
    W = H * hd
    q, k, v = (torch.randn(G0, G1, n, W, generator=g) * mag for n in (Nq, Nk, Nk))
    return (q, k, v) + A64.attention64(q, k, v, H)


@pytest.mark.parametrize("G0,G1", GROUPS)
@pytest.mark.parametrize("Nq,Nk,hd,H", SHAPES)
def test_per_element_against_fp64(Nq, Nk, hd, H, G0, G1):
    from gd_amd import ops
    for mag in (1.0, 4.0, 6.0):
        q, k, v, want, bound = dense_case(Nq, Nk, hd, H, G0, G1, mag)
        got = ops.attention_small_fwd(q.cuda(), k.cuda(), v.cuda(), G0, G1, Nq, Nk, H).cpu()
        r, e, b = worst(got, want, bound)
        print(f"attention_small Nq={Nq} Nk={Nk} hd={hd} H={H} G=({G0},{G1}) inputs x{mag:g}: worst err / bound {r:.4f} (err {e:.2e}, bound {b:.2e})")
        assert got.shape == (G0, G1, Nq, H * hd) and got.is_contiguous() and bool(torch.isfinite(got).all()) and r <= 1.0


# ---------------------------------------------------------------------------------------------------------------------------------- addressing
SENTINEL = -12345.678


def strided_run(flats, offs, G0, G1, Nq, Nk, H, hd, lds, strides, oflat, ooff, ldo, so):
    """Runs the wrapper on as_strided views of flat device buffers; -> nothing (oflat is written in place)."""
    from gd_amd import ops
    W = H * hd
    view = lambda f, off, n, ld, st: torch.as_strided(f, (G0, G1, n, W), (st[0], st[1], ld, 1), off)
    ops.attention_small_fwd(view(flats[0], offs[0], Nq, lds[0], strides[0]), view(flats[1], offs[1], Nk, lds[1], strides[1]),
                            view(flats[2], offs[2], Nk, lds[2], strides[2]), G0, G1, Nq, Nk, H, out=view(oflat, ooff, Nq, ldo, so))


def poisoned(flat, off, G0, G1, n, W, st, ld):
    """A copy of `flat` with NaN in every cell the operand does NOT address."""
    out = torch.full_like(flat, float("nan"))
    c = A64.cells(off, G0, G1, n, W, st[0], st[1], ld)
    out[c] = flat[c]
    return out


def check_strided(name, srcs, offs, G0, G1, Nq, Nk, H, hd, lds, strides, osize, ooff, ldo, so):
    """srcs: the flat buffers q, k and v are read from.  Each operand gets its own copy with NaN in every cell it does not address; the output buffer is
    full of a sentinel, which every cell outside the addressed ones must still hold bit for bit."""
    W = H * hd
    ns = (Nq, Nk, Nk)
    flats = [poisoned(srcs[i], offs[i], G0, G1, ns[i], W, strides[i], lds[i]) for i in range(3)]
    want, bound = A64.attention_strided64(*flats, offs, G0, G1, Nq, Nk, H, hd, lds, strides)
    oflat = torch.full((osize,), SENTINEL).cuda()
    strided_run([f.cuda() for f in flats], offs, G0, G1, Nq, Nk, H, hd, lds, strides, oflat, ooff, ldo, so)
    oflat = oflat.cpu()
    c = A64.cells(ooff, G0, G1, Nq, W, so[0], so[1], ldo)
    got = oflat[c].view(G0, G1, Nq, W)
    r, e, b = worst(got, want, bound)
    print(f"attention_small {name}: worst err / bound {r:.4f} (err {e:.2e}, bound {b:.2e}); {c.numel()} of {osize} output cells addressed")
    assert bool(torch.isfinite(got).all()) and r <= 1.0
    untouched = torch.ones(osize, dtype=torch.bool)
    untouched[c] = False
    assert bool((oflat[untouched].view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32)).all()), "a cell outside the addressed ones was written"


@pytest.mark.parametrize("hd,S", [(12, 3), (48, 2)])
def test_time_stage_packed_column_blocks(hd, S):
    """q | k | v are column blocks of ONE packed [rows, 3 D (+ pad)] tensor, sequences of S consecutive rows; o is [rows, D (+ pad)]."""
    H, rows = 8, 2 * (5 + 4)
    D = H * hd
    ld, ldo = 3 * D + 8, D + 4
    flat = torch.randn(rows * S * ld, generator=gen(hd))
    check_strided(f"time stage hd={hd} S={S}", (flat,) * 3, (0, D, 2 * D), rows, 1, S, S, H, hd, (ld,) * 3, ((S * ld, 0),) * 3, rows * S * ldo, 0, ldo,
                  (S * ldo, 0))


@pytest.mark.parametrize("hd", [12, 48])
@pytest.mark.parametrize("stage", ["virtual2point", "virtual", "point2virtual"])
def test_space_stage_addressing(hd, stage):
    """One token layout [B, N + nv, S, ld], rows (b, n, s): the tokens of frame (b, s) are S * ld apart, points from offset 0 of a batch entry,
    virtual rows from N * S * ld.  q from a [.., D (+ pad)] buffer of that layout, k | v column blocks of a [.., 2 D (+ pad)] one, o into a third."""
    B, S, N, nv, H = 2, 3, 5, 4, 8
    D = H * hd
    ldq, ldkv, ldo = D + 8, 2 * D + 4, D + 12
    n = N + nv
    qflat, kvflat = torch.randn(B * n * S * ldq, generator=gen(1)), torch.randn(B * n * S * ldkv, generator=gen(2))
    off = lambda ld, virtual: N * S * ld if virtual else 0
    qv, kv, Nq, Nk = {"virtual2point": (True, False, nv, N), "virtual": (True, True, nv, nv), "point2virtual": (False, True, N, nv)}[stage]
    st = lambda ld: (n * S * ld, ld)
    check_strided(f"space stage {stage} hd={hd}", (qflat, kvflat, kvflat), (off(ldq, qv), off(ldkv, kv), off(ldkv, kv) + D), B, S, Nq, Nk, H, hd,
                  (S * ldq, S * ldkv, S * ldkv), (st(ldq), st(ldkv), st(ldkv)), B * n * S * ldo, off(ldo, qv), S * ldo, st(ldo))


# ---------------------------------------------------------------------------------------------------------------------------------- softmax range
@pytest.mark.parametrize("Nq,Nk,hd,H", [(2, 2, 48, 8), (17, 65, 48, 8), (64, 300, 12, 3)])
def test_large_logits_and_equal_scores(Nq, Nk, hd, H):
    from gd_amd import ops
    G0, G1, W = 3, 2, H * hd
    g = gen(Nk)
    q, k, v = (torch.randn(G0, G1, n, W, generator=g) for n in (Nq, Nk, Nk))
    # scaled so that the largest |score| is about 80 (a spread of up to 160 between two scores of a row: exp of it overflows fp32 unless the running
    # maximum is subtracted, and the weights far below the maximum flush to zero)
    s = (q.view(G0, G1, Nq, H, hd).transpose(2, 3).double() @ k.view(G0, G1, Nk, H, hd).transpose(2, 3).double().transpose(-1, -2)) * hd ** -0.5
    f = (80.0 / float(s.abs().max())) ** 0.5
    q, k = q * f, k * f
    want, bound = A64.attention64(q, k, v, H)
    got = ops.attention_small_fwd(q.cuda(), k.cuda(), v.cuda(), G0, G1, Nq, Nk, H).cpu()
    r, e, b = worst(got, want, bound)
    smax = float((s * f * f).abs().max())
    print(f"attention_small Nq={Nq} Nk={Nk} hd={hd}: max |score| {smax:.1f}: worst err / bound {r:.4f} (err {e:.2e}, bound {b:.2e})")
    assert 79.0 <= smax <= 81.0 and bool(torch.isfinite(got).all()) and r <= 1.0
    # all scores of a query equal (every key row the same): the output is the mean of v
    k1 = k[:, :, :1].expand(G0, G1, Nk, W).contiguous()
    want, bound = A64.attention64(q, k1, v, H)
    got = ops.attention_small_fwd(q.cuda(), k1.cuda(), v.cuda(), G0, G1, Nq, Nk, H).cpu()
    r, e, b = worst(got, want, bound)
    print(f"attention_small Nq={Nq} Nk={Nk} hd={hd}: equal scores: worst err / bound {r:.4f} (err {e:.2e}, bound {b:.2e})")
    assert bool(torch.isfinite(got).all()) and r <= 1.0
    assert float((want - v.double().mean(2, keepdim=True)).abs().max()) <= 1e-12


def test_two_runs_are_bit_identical():
    from gd_amd import ops
    for Nq, Nk, hd, H, G0, G1 in ((2, 2, 48, 8, 41, 1), (64, 300, 48, 8, 1, 2), (300, 64, 48, 8, 1, 2), (33, 129, 12, 3, 3, 2)):
        q, k, v, _, _ = dense_case(Nq, Nk, hd, H, G0, G1, 1.0)
        q, k, v = q.cuda(), k.cuda(), v.cuda()
        a = ops.attention_small_fwd(q, k, v, G0, G1, Nq, Nk, H)
        junk = torch.full_like(a, float("nan"))
        del junk
        b = ops.attention_small_fwd(q, k, v, G0, G1, Nq, Nk, H)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (Nq, Nk)


def test_scale_and_out_arguments():
    from gd_amd import ops
    q, k, v, _, _ = dense_case(15, 17, 48, 2, 3, 2, 1.0)
    want, bound = A64.attention64(q, k, v, 2, scale=0.3)
    out = torch.empty(3, 2, 15, 96 + 8, device="cuda")[..., :96]
    got = ops.attention_small_fwd(q.cuda(), k.cuda(), v.cuda(), 3, 2, 15, 17, 2, scale=0.3, out=out)
    assert got is out
    r, e, b = worst(got.cpu(), want, bound)
    print(f"attention_small scale=0.3, out= a pitched view: worst err / bound {r:.4f}")
    assert r <= 1.0
