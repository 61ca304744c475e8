"""CPU: the fp64 restatement, the probe inputs and the derived bounds of tests/cv_ref64.py, before tests/test_gpu_cost_volume_paths.py relies on them.
(1) The restatement (loss; gradients as a function of the stats it saves) equals fp64 autograd of oracle/gd_oracle.py::cost_volume_kl for both
variants, masked rows and the clamped teacher rows included.  (2) The probe conditions hold: the exact-score features give scores in {-1, 0, 1} exactly in
bf16, fp16, fp32 and in the three-way bf16 split, Z equals its closed form from counts, a dropped or doubled column moves logZ by more than FACTOR times
its bound at every size used, the selector keeps one row per (pair, view) at a tile edge with a nonzero selected score, and the random family's cosines
cover [-0.9, 0.9].  (3) Every mutant of the restatement breaks at least one bound (loss, logZ, df1, df2) by a factor >= 4 in at least one input family,
at every (kind, C, hw) of the GPU file's case table.  GD_CV_MUTANTS=<file>: the smallest factor of every mutant is written there; it is printed too."""
import math
import os

import pytest
import torch

import cv_ref64 as R
import gd_oracle as O
import test_gpu_cost_volume_paths as G

FACTOR = 4.0
_MIN = {}
# every (kind, C, hw, kcap) the GPU file runs the restatement at: the dense case table, the kept-row table, the long forward
POINTS = sorted({(c["kind"], c["C"], hw, 0) for c, hw in G.DENSE} | {(k, C, hw, kcap) for k, C, hw, kcap in G.ROWS}) + [("f32", 32, 1537, 0)]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"{_MIN[k][0]:12.1f}  {k:28s} smallest at {_MIN[k][1]}" for k in sorted(_MIN)]
    print("\n".join(["smallest factor by which each mutant exceeds a bound:"] + lines))
    path = os.environ.get("GD_CV_MUTANTS")
    if path and _MIN:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


def _oracle(x, variant):
    fa, fb = [t.double() for t in x.operands()]
    losses, g1, g2 = [], [], []
    for p in range(x.P):
        a, b = fa[p:p + 1].clone().requires_grad_(True), fb[p:p + 1].clone().requires_grad_(True)
        l = O.cost_volume_kl(a, b, x.t1[p:p + 1].double(), x.t2[p:p + 1].double(), x.m1[p], x.m2[p], variant)
        (l * x.gloss[p].double()).backward()
        losses.append(l.detach())
        g1.append(a.grad[0])
        g2.append(b.grad[0])
    return torch.stack(losses), torch.stack(g1), torch.stack(g2)


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("hw,C", [(1, 8), (5, 8), (65, 40), (129, 64), (257, 96)])
def test_restatement_equals_oracle_autograd(hw, C, family, variant):
    x = R.make_inputs(family, 3, hw, C, "bf16")          # (bf16: the masters ARE the operands, and the oracle sees the same rows)
    f = R.forward64(x, variant)
    ol, og1, og2 = _oracle(x, variant)
    assert float((f["loss"] - ol).abs().max()) <= 1e-12 * max(1.0, float(ol.abs().max()))
    d1, d2, b1, b2 = R.backward64(x, f["stats"])
    for got, ref in ((d1, og1), (d2, og2)):
        assert float((got - ref).abs().max()) <= 1e-11 * max(float(ref.abs().max()), 1e-30)
    for b in (f["b_loss"], f["b_stats"], b1, b2):
        assert bool(torch.isfinite(b).all()) and float(b.min()) >= 0.0
    ts, tb = R.teacher_stats64(x)
    g = R.forward64(x, variant, inv=x.inv32(), tstats=ts.float())          # the GIVEN-statistics form restates the same operation
    assert float((g["loss"] - f["loss"]).abs().max()) <= 1e-5 * max(1.0, float(f["loss"].abs().max()))


def _split3(v):
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    return hi, lo


@pytest.mark.parametrize("kind,C,hw,kcap", POINTS)
def test_probe_input_conditions(kind, C, hw, kcap):
    P = 1 if hw > 1000 else 3
    x = R.make_inputs("exact", P, hw, C, kind)
    for dt in (torch.bfloat16, torch.float16, torch.float32):
        if kind == "f16" or dt != torch.float16:          # (the f32 / bf16 probes use exponents down to -8 and up to 8: inside fp16 too, checked anyway)
            assert torch.equal(x.f1.to(dt).float(), x.f1) and torch.equal(x.f2.to(dt).float(), x.f2)
    inv1, inv2 = x.inv32()
    # fp32 arithmetic as the kernels run it: the dot products, then the two scalings, every step exact
    S32 = (x.f1 @ x.f2.transpose(-1, -2)) * inv1[:, :, None] * inv2[:, None, :]
    assert bool(((S32 == 0) | (S32.abs() == 1)).all())
    h1, l1 = _split3(x.f1)
    h2, l2 = _split3(x.f2)
    assert float(l1.abs().max()) == 0.0 and float(l2.abs().max()) == 0.0 and torch.equal(h1, x.f1) and torch.equal(h2, x.f2)      # the split is the value itself
    f = R.forward64(x, "vggt", inv=(inv1, inv2))
    assert torch.equal(f["stats"][:, 0, :, 0] * x.f1.double().norm(dim=-1), torch.ones(P, hw, dtype=torch.float64))
    S = S32.double()
    for d, Sd in enumerate((S, S.transpose(-1, -2))):
        npos, nneg, nzero = (Sd == 1).sum(-1).double(), (Sd == -1).sum(-1).double(), (Sd == 0).sum(-1).double()
        Z = npos * math.e + nzero + nneg / math.e
        assert float((f["stats"][:, d, :, 2] - Z.log()).abs().max()) <= 1e-12
        if hw >= 64:
            assert len({(int(a), int(b)) for a, b in zip(npos[0], nneg[0])}) >= min(C, 7)          # the counts differ from row to row: one class per (axis, sign)
        # detectability: one column more or less moves Z by at least 1 / e, logZ by at least 1 / (e Z) >= 1 / (hw e^2)
        move = (1.0 / (math.e * Z)).clamp_max(0.5)
        assert bool((move >= 1.0 / (hw * math.e ** 2) - 1e-15).all())
        assert bool((move >= FACTOR * f["b_stats"][:, d, :, 2]).all()), (kind, C, hw, float((move / f["b_stats"][:, d, :, 2]).min()))
    s = R.make_inputs("selector", P, hw, C, kind)
    pi = R._perm(hw)
    assert sorted(pi.tolist()) == list(range(hw))
    if hw >= 257:
        assert any(int(pi[i]) // 128 != i // 128 for i in range(hw)) and any(int(pi[i]) // 64 != i // 64 for i in range(hw))
    i1, i2 = s.inv32()
    Ss = (s.f1 @ s.f2.transpose(-1, -2)) * i1[:, :, None] * i2[:, None, :]
    assert bool(((Ss == 0) | (Ss.abs() == 1)).all())
    for p, (r1, r2) in enumerate(R.select_rows(hw, P)):
        assert int(s.m1[p].sum()) == 1 and int(s.m2[p].sum()) == 1 and bool(s.m1[p, r1]) and bool(s.m2[p, r2])
        assert abs(float(Ss[p, r1, pi[r1]])) == 1.0 and (hw == 1 or abs(float(Ss[p, pi[r2], r2])) == 1.0), (p, r1, r2)
    if hw >= 129:
        assert {r for rr in R.select_rows(hw, P) for r in rr} >= ({0, 63, 64, 127, 128, hw - 1} if P == 3 else {0, 63})
    if hw >= 65 and C >= 8:
        r = R.make_inputs("random", P, hw, C, kind)
        a, b = [t.double() for t in r.operands()]
        an, bn = a / a.norm(dim=-1, keepdim=True).clamp_min(1e-300), b / b.norm(dim=-1, keepdim=True).clamp_min(1e-300)
        cos = an @ bn.transpose(-1, -2)
        assert float(cos.min()) <= -0.85 and float(cos.max()) >= 0.85, (float(cos.min()), float(cos.max()))
        nr = a.norm(dim=-1)
        nr = nr[nr > 0]
        assert float(nr.max() / nr.min()) >= (20.0 if kind == "f16" else 1e3)
        assert float(a.abs().max()) < 65504.0


def _note(mutant, factor, where):
    if mutant not in _MIN or factor < _MIN[mutant][0]:          # (inf: a NaN or an overflow, e.g. the wrong inverse norm of a zero feature row)
        _MIN[mutant] = (factor, where)


@pytest.mark.parametrize("kind,C,hw,kcap", POINTS)
def test_every_mutant_exceeds_a_bound(kind, C, hw, kcap):
    """The forward mutants are run through forward64, all of them through backward64 on the stats of the UNMUTATED forward (what the kernels would be
    given); a mutant's factor at this point is the largest err / bound over loss, logZ, df1, df2 and the input families."""
    P = 1 if hw > 1000 else 3
    families = ("exact", "selector") if hw > 1000 else R.FAMILIES
    best, finite, expected_gaps = {}, {}, None
    for family in families:
        x = R.make_inputs(family, P, hw, C, kind)
        if kcap and family != "selector":
            x = G._with_kept_counts(x, G.KEPT_COUNTS)
        inv = x.inv32()
        ts, _ = R.teacher_stats64(x)
        ts = ts.float()
        ref = R.forward64(x, "mast3r", inv=inv, tstats=ts)
        stats = ref["stats"].float()
        keep = torch.stack([x.m1, x.m2], 1)
        rb = R.backward64(x, stats, kcap=kcap) if hw <= 1000 else None
        for name, m in R.mutants(x):
            if m is None:
                continue
            f = R.forward64(x, "mast3r", inv=inv, tstats=ts, mut=m)
            r = [R.ratio(f["loss"], ref["loss"], ref["b_loss"])[0]]
            lz, lr, lb = f["stats"][..., 2], ref["stats"][..., 2], ref["b_stats"][..., 2]
            r.append(R.ratio(lz[keep], lr[keep], lb[keep])[0] if kcap else R.ratio(lz, lr, lb)[0])
            if rb is not None:
                mb = R.backward64(x, stats, mut=m, kcap=kcap)
                r += [R.ratio(mb[0], rb[0], rb[2])[0], R.ratio(mb[1], rb[1], rb[3])[0]]
            best[name] = max(best.get(name, 0.0), max(r))
            finite[name] = max([finite.get(name, 0.0)] + [v for v in r if math.isfinite(v)])
        gaps = {n for n, m in R.mutants(x) if m is None}
        expected_gaps = gaps if expected_gaps is None else expected_gaps & gaps
    # the only points where a mutant IS the reference in every family: no ragged edge, no pad, one row, one tile
    allowed = set()
    if hw == 1:
        allowed |= {"drop_student_col", "t1_for_direction_2", "inv_of_other_view", "kept_index_off_by_one"}
    if hw <= 128:
        allowed.add("skip_128_tile")
    if hw % 128 == 0:
        allowed.add("ragged_col_live")
    if hw % 64 == 0:
        allowed.add("G_pad_nonzero")
    if P == 1:
        allowed.add("neighbour_pair_stats")
    assert expected_gaps <= allowed, (expected_gaps - allowed)
    # ... and three points where a mutant differs from the reference by less than fp32 can show, by the operation itself: with one column p = t = 1, so
    # G is zero whatever its pad holds and a kept row's KL term is zero like a masked row's; the masked rows' constant hw 1e-8 log(1e-8 hw) is below
    # the rounding of an O(1) loss for hw < 63 (it reaches FACTOR bounds from hw = 63 on); only the forward runs at the long size, so its
    # backward-only mutants have nothing to show in.
    waived = ({"G_pad_nonzero", "masked_as_kept", "kept_as_masked"} if hw == 1 else set()) | ({"vggt_const_for_mast3r"} if hw < 63 else set()) | \
        ({"G_pad_nonzero", "neighbour_pair_stats"} if hw > 1000 else set())
    for name, factor in best.items():
        if name in waived:
            continue
        # reported: the largest FINITE factor where one reaches FACTOR (an overflow to inf or NaN in another family says less about the bound)
        _note(name, finite[name] if finite[name] >= FACTOR else factor, f"{kind} C={C} hw={hw}" + (f" kcap={kcap}" if kcap else ""))
        assert factor >= FACTOR, (name, kind, C, hw, kcap, factor)
