"""tests/loss_ref64.py checked on the CPU: its explicit fp64 gradients against autograd of the same formulas written with torch's own layer_norm / gelu,
its values against gd_oracle where the oracle covers the case, and that the bounds are tight enough AT THE GPU TESTS' OWN INPUTS for a list of wrong
restatements to fail them by 4 x at some element, for every valid pair of the ranking inputs to matter, and for no comparison to be ambiguous."""
import functools

import gd_oracle as O
import pytest
import torch
import torch.nn.functional as F

import loss_ref64 as L

F64 = torch.float64


def _worst(wrong, ref):
    """max over the elements of |wrong - ref| / bound (bound 0: any difference is infinite)."""
    w = wrong.v if isinstance(wrong, L.V) else wrong
    err, b = (w - ref.v).abs(), L.bound(ref)
    r = torch.where(b > 0, err / b, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max()) if r.numel() else 0.0


def _close(a, b, what, rel=1e-12):
    scale = max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= rel * scale, f"{what}: {float((a - b).abs().max()) / scale:.3e} relative"


def _hp64(hp, grad=False):
    return {k: v.double().clone().requires_grad_(grad) for k, v in hp.items()}


def _head_torch(z, hp):
    h = F.gelu(F.layer_norm(z, (128,), hp["ln_w"], hp["ln_b"], 1e-5))
    return torch.tanh(h @ hp["w2"] + hp["b2"][0])


def _hg_torch(hp):
    return torch.cat([hp[k].grad.reshape(-1) for k in ("b1", "ln_w", "ln_b", "w2", "b2")])


@functools.lru_cache(maxsize=None)
def _rank(name, head):
    inp = L.rank_inputs(name, head)
    return inp, L.rank_case(inp)


# ------------------------------------------------------------------------------------------------ explicit gradients are autograd's
@pytest.mark.parametrize("head", L.HEAD_NAMES)
def test_ranking_gradients_equal_autograd(head):
    inp = L.rank_inputs("ragged_1", head)
    n = 12
    u = inp.u[0, :n].double().requires_grad_(True)
    hp = _hp64(inp.hp, True)
    dd = inp.depth[0, :n].double()[None] - inp.depth[0, :n].double()[:, None]
    valid = dd.abs() > L.f32(inp.thr)
    s = _head_torch(u[None] - u[:, None] + hp["b1"], hp)
    loss = torch.log(1 + torch.exp(-torch.sign(dd) * s))[valid].mean()
    (loss * 0.75).backward()
    r = L.rank_set(inp.u[0, :n], inp.depth[0, :n], inp.thr, inp.hp, 0.75)
    assert r["cnt"] == int(valid.sum())
    _close(r["loss"].v, loss.detach(), "loss")
    _close(r["du"].v, u.grad, "du")
    _close(r["hg"].v[:513], _hg_torch(hp), "head gradients")
    assert not r["hg"].v[513:].any() and not r["hg"].e[513:].any()


def test_l1_and_head_row_gradients_equal_autograd():
    inp = L.l1_inputs()
    ref = L.l1_case(inp)
    hp = _hp64(inp.hp, True)
    u = inp.u.double().requires_grad_(True)
    tot = 0
    for p in range(4):
        n = inp.n(p)
        if n == 0:
            assert ref["loss"].v[p] == 0 and not ref["hg_sets"].v[p].any()
            continue
        s = _head_torch(u[p, 0, :n] - u[p, 1, :n] + hp["b1"], hp)
        l1 = (s - torch.tanh(inp.d1[p, :n].double() - inp.d2[p, :n].double())).abs().mean()
        _close(ref["loss"].v[p], l1.detach(), f"l1 loss {p}")
        tot = tot + l1 * L.f32(float(inp.gscale[p]))
    tot.backward()
    _close(ref["du"].v, u.grad, "l1 du")
    _close(ref["hg_sum"].v[:513], _hg_torch(hp), "l1 head gradients")
    rows, dout, hpr = L.head_inputs(33)
    hp = _hp64(hpr, True)
    x = rows.double().requires_grad_(True)
    out = _head_torch(x + hp["b1"], hp)
    (out * dout.double()).sum().backward()
    s, du, hg = L.head_rows(rows, hpr, dout)
    _close(s.v, out.detach(), "head rows")
    _close(du.v, x.grad, "head rows du")
    _close(hg.v[:513], _hg_torch(hp), "head rows head gradients")


def _sig(x, temp):
    return 1.0 / (1.0 + torch.exp(torch.clamp(-x * L.inv_temp(temp), -50.0, 50.0)))      # clamp's own autograd is zero outside


@pytest.mark.parametrize("variant", [0, 1])
def test_smooth_ap_gradients_equal_autograd(variant):
    inp = L.ap_inputs("small")
    for p in range(2):
        s = inp.sim[p].double().requires_grad_(True)
        n = s.shape[0]
        neg = ((L._dist(inp.p1[p], inp.p2[p]) > L.f32(inp.thr_neg)) & ~torch.eye(n, dtype=torch.bool)).double()
        pos = s.diagonal()
        r1 = _sig(1 - pos if variant == 0 else pos - 1, inp.temp) + 1
        r2 = _sig(1 - pos, inp.temp) + 1
        ap1 = r1 / (r1 + (_sig(s - 1, inp.temp) * neg).sum(1))
        ap2 = r2 / (r2 + (_sig(s - pos[:, None], inp.temp) * neg).sum(1))
        loss = (1 - (ap1 + ap2) / 2).mean()
        loss.backward()
        rows, dsim = L.ap_pair(inp.sim[p], inp.p1[p], inp.p2[p], variant, inp.thr_neg, inp.temp)
        _close(rows.v.sum(), loss.detach(), "smooth-AP loss")
        _close(dsim.v, s.grad, "dsim")


def test_smooth_ap_me_gradients_equal_autograd():
    inp = L.ap_inputs("small", me=True)
    s = inp.sim[0].double().requires_grad_(True)
    d = L._dist(inp.p1[0], inp.p2[0])
    neg = (d > L.f32(inp.thr_neg)).double()
    ii, jj = torch.nonzero(d < L.f32(inp.thr_pos), as_tuple=True)
    pos = s[ii, jj]
    r1, r2 = _sig(pos - 1, inp.temp) + 1, _sig(1 - pos, inp.temp) + 1
    ap1 = r1 / (r1 + (_sig(s[ii] - 1, inp.temp) * neg[ii]).sum(1))
    ap2 = r2 / (r2 + (_sig(s[ii] - pos[:, None], inp.temp) * neg[ii]).sum(1))
    loss = (1 - (ap1 + ap2) / 2).mean()
    loss.backward()
    ls, rows, dsim = L.me_pair(inp.sim[0], inp.p1[0], inp.p2[0], inp.thr_pos, inp.thr_neg, inp.temp)
    assert sorted(set(rows.v[:, 1].long().tolist())) == [0, 1, 3], "rows with 0, 1 and 3 positives"
    _close(ls.v, loss.detach(), "ME loss")
    _close(dsim.v, s.grad, "ME dsim")
    ls, rows, dsim = L.me_pair(inp.sim[1], inp.p1[1], inp.p2[1], inp.thr_pos, inp.thr_neg, inp.temp)      # the pair without any positive
    assert ls.v == 0 and not dsim.v.any() and not dsim.e.any() and not rows.v.any()


# ------------------------------------------------------------------------------------------------ the oracle
def test_restatements_agree_with_the_oracle():
    inp = L.l1_inputs(with_gscale=False)
    hp = _hp64(inp.hp)
    hp["w1"], hp["w2"] = torch.eye(128, dtype=F64), hp["w2"][None]
    ref = L.l1_case(inp)
    rk = L.RankInputs("l1 views", inp.u.reshape(8, 21, 128), torch.stack([inp.d1, inp.d2], 1).reshape(8, 21), inp.counts.repeat_interleave(2), None,
                      L.RANK_THR, inp.hp)
    rr = L.rank_case(rk)
    for p in range(3):
        n = inp.n(p)
        l1, intra = O.depth_losses(hp, inp.u[p, 0:1, :n].double(), inp.u[p, 1:2, :n].double(), inp.d1[p:p + 1, :n].double(), inp.d2[p:p + 1, :n].double())
        _close(ref["loss"].v[p], l1, "oracle l1")
        _close(0.5 * (rr["loss"].v[2 * p] + rr["loss"].v[2 * p + 1]), intra, "oracle ranking")
    g = torch.Generator().manual_seed(1)
    d1 = F.normalize(torch.randn(1, 20, 16, generator=g, dtype=F64), dim=-1)
    d2 = F.normalize(d1 + 0.05 * torch.randn(1, 20, 16, generator=g, dtype=F64), dim=-1)
    p1 = torch.rand(1, 20, 3, generator=g)
    p2 = p1 + 1e-3 * torch.randn(1, 20, 3, generator=g)
    sim = (d1 @ d2.transpose(1, 2))[0]
    for variant, name in ((0, "vggt"), (1, "mast3r")):
        rows, _ = L.ap_pair(sim, p1[0], p2[0], variant, 0.1, 0.01)
        _close(rows.v.sum(), O.smooth_ap_loss(d1, d2, p1.double(), p2.double(), name), f"oracle smooth-AP {name}", 1e-9)
    p2[0, 3], p2[0, 4] = p1[0, 2] + 1e-3, p1[0, 2] - 1e-3
    ls, _, _ = L.me_pair(sim, p1[0], p2[0], 5e-3, 0.1, 0.01)
    _close(ls.v, O.smooth_ap_loss_me(d1, d2, p1.double(), p2.double()), "oracle ME", 1e-9)


# ------------------------------------------------------------------------------------------------ the inputs are what the GPU tests need
@pytest.mark.parametrize("name", list(L.RANK_CASES))
def test_ranking_inputs(name):
    """No pair within 1e-5 of the threshold (the exact case: only pairs AT it, which its exact subtraction decides); the seam pair valid in the sets
    that hold it; ln_w, ln_b, b2 not trivial.  "active" head: every valid ordered pair moves a du element by more than 4 x its bound.  "saturating"
    head: the pre-tanh value of the valid pairs spans more than [-4, 4] — there the pairs near +-4 are below the bound of their row sums (printed),
    which is why the case has two heads."""
    for head in L.HEAD_NAMES:
        inp, ref = _rank(name, head)
        assert L.ambiguous_pairs(inp.depth, inp.counts, inp.thr) == 0
        assert (inp.hp["ln_w"] - 1).abs().max() > 0.3 and inp.hp["ln_b"].abs().max() > 0.2 and float(inp.hp["b2"]) != 0
        lo, hi, worst, below = 1e9, -1e9, 1e9, 0
        for s in range(inp.S):
            n = inp.n(s)
            g = 1.0 if inp.gscale is None else float(inp.gscale[s])
            r = L.rank_set(inp.u[s, :n], inp.depth[s, :n], inp.thr, inp.hp, g, want_pairs=True)
            assert r["cnt"] == ref["cnt"][s]
            if n < 2:
                assert r["cnt"] == 0
                continue
            if n > L.SEAM_PAIR[1] and name != "exact_mask":
                assert r["valid"][L.SEAM_PAIR] and r["valid"][L.SEAM_PAIR[::-1]]
            ov = r["o"][r["valid"]]
            lo, hi = min(lo, float(ov.min())), max(hi, float(ov.max()))
            if g != 0:
                ratio, valid = L.pair_ratios(r, L.bound(r["du"]))
                worst, below = min(worst, float(ratio[valid].min())), below + int((ratio[valid] <= 4).sum())
        print(f"{name} {head}: pre-tanh of the valid pairs in [{lo:.2f}, {hi:.2f}], smallest pair contribution / bound {worst:.2f}, pairs <= 4: {below}")
        if head == "active":
            assert worst > 4.0 and below == 0
        else:
            assert lo < -4.0 and hi > 4.0
    if name == "exact_mask":
        inp, _ = _rank(name, "active")
        dd = (inp.depth[0][None] - inp.depth[0][:, None]).abs()
        off = ~torch.eye(40, dtype=torch.bool)
        assert (dd == 0.25).any() and (dd[off] == 0).any() and (dd > 0.25).any()
        assert torch.equal(inp.u[:, 3], inp.u[:, 0]) and (inp.depth[:, 3] != inp.depth[:, 0]).all()
        assert torch.equal((inp.depth.double()[:, None] - inp.depth.double()[:, :, None]).float().double(),
                           inp.depth.double()[:, None] - inp.depth.double()[:, :, None]), "every fp32 subtraction is exact"


def test_l1_and_smooth_ap_inputs_have_no_ambiguous_comparison():
    for fs in (1.0, 0.05):
        assert L.ambiguous_l1(L.l1_case(L.l1_inputs(fs))["resid"]) == 0
    for shape in L.AP_SHAPES:
        for me in (False, True):
            inp = L.ap_inputs(shape, me)
            assert L.ambiguous_ap(inp, me) == 0
            assert float(inp.sim.diagonal(dim1=1, dim2=2).min()) >= 0.7 and float(inp.sim.diagonal(dim1=1, dim2=2).max()) <= 1.0
    inp = L.ap_inputs("stride")
    n = 256
    s, inv = inp.sim[2, :n, :n].double(), L.inv_temp(inp.temp)
    for x in ((s - 1) * inv, (s - s.diagonal()[:, None]) * inv):
        off = x[~torch.eye(n, dtype=torch.bool)].abs()
        assert (off < 5).any() and (off > 60).any() and ((off > 49.9) & (off < 50)).any() and ((off > 50) & (off < 50.1)).any()
    d = L._dist(inp.p1[0], inp.p2[0])
    assert d[2, 3] == 0 and d[1, 1] > inp.thr_neg
    me = L.me_case(L.ap_inputs("stride", me=True))
    assert sorted(set(me["rows"].v[0, :, 1].long().tolist())) == [0, 1, 3] and not me["rows"].v[1, :, 1].any() and me["loss"].v[1] == 0


# ------------------------------------------------------------------------------------------------ wrong restatements fail the bounds
RANK_MUTANTS = [("exact_mask", dict(mask_ge=True), ">= in the depth mask"),
                ("ragged_1", dict(drop_mirror=True), "the mirrored pair dropped from du_i"),
                ("seams_full", dict(drop_pair=L.SEAM_PAIR), "one valid pair dropped at a tile seam"),
                ("ragged_1", dict(drop_pair=L.SEAM_PAIR), "one valid pair dropped at a tile seam"),
                ("seams_counts", dict(mean_n2=True), "mean over n^2"),
                ("ragged_0.05", dict(eps=1e-6), "LayerNorm eps 1e-6"),
                ("ragged_0.05", dict(gelu="tanh"), "tanh-form GELU"),
                ("ragged_1", dict(swap_ln=True), "ln_w and ln_b gradients swapped")]


@pytest.mark.parametrize("name,mut,what", RANK_MUTANTS, ids=[m[2].replace(" ", "_") + "-" + m[0] for m in RANK_MUTANTS])
def test_wrong_rankings_fail_the_bound(name, mut, what):
    for head in L.HEAD_NAMES if "drop_pair" not in mut else ("active",):          # (a saturated pair's gradient is below its row's bound)
        inp, ref = _rank(name, head)
        wrong = L.rank_case(inp, **mut)
        got = {k: _worst(wrong[k], ref[k]) for k in ("loss", "du", "hg_sets")}
        print(f"{what} [{name}, {head}]: worst err / bound {got}")
        key = "hg_sets" if "swap_ln" in mut else "du"
        assert got[key] >= 4.0, (what, head, got)
        if "mask_ge" in mut or "mean_n2" in mut:
            assert got["loss"] >= 4.0, (what, head, got)
        if "mask_ge" in mut:
            assert wrong["cnt"] != ref["cnt"]
    for k in ("loss", "du", "hg_sets"):
        assert _worst(ref[k].v.float().double(), ref[k]) <= 1.0, "the correctly rounded result is inside the bound"


def test_wrong_heads_fail_the_l1_and_row_bounds():
    for fs in (1.0, 0.05):
        inp = L.l1_inputs(fs)
        ref = L.l1_case(inp)
        for mut in (dict(eps=1e-6), dict(gelu="tanh")):
            wrong = L.l1_case(inp, **mut)
            got = {k: _worst(wrong[k], ref[k]) for k in ("loss", "du", "hg_sets")}
            print(f"l1 {mut} scale {fs}: {got}")
            if fs == 0.05 or "gelu" in mut:                     # (eps 1e-6 against a variance near 2 is inside the bounds, as it should be)
                assert got["du"] >= 4.0 and got["hg_sets"] >= 4.0
    for M in L.HEAD_M:
        rows, dout, hp = L.head_inputs(M, 0.05)
        s, du, hg = L.head_rows(rows, hp, dout)
        for mut in (dict(eps=1e-6), dict(gelu="tanh")):
            ws, wdu, whg = L.head_rows(rows, hp, dout, **mut)
            assert _worst(ws, s) >= 4.0 and _worst(wdu, du) >= 4.0 and ("eps" in mut or _worst(whg, hg) >= 4.0), (M, mut)
        swapped = torch.cat([hg.v[:128], hg.v[256:384], hg.v[128:256], hg.v[384:]])
        assert _worst(swapped, hg) >= 4.0


@pytest.mark.parametrize("shape", list(L.AP_SHAPES))
def test_wrong_smooth_ap_fails_the_bound(shape):
    inp = L.ap_inputs(shape)
    for variant in (0, 1):
        ref = L.ap_case(inp, variant)
        for mut, what in ((dict(zero_outside=False), "saturated derivative not zeroed"), (dict(diag_neg=True), "diagonal counted as a negative"),
                          (dict(swap_variant=True), "variants swapped in rpos1")):
            wrong = L.ap_case(inp, variant, **mut)
            got = {k: _worst(wrong[k], ref[k]) for k in ("loss", "rows", "dsim")}
            print(f"{what} [{shape}, variant {variant}]: {got}")
            assert got["dsim"] >= 4.0, what
            if "zero_outside" not in mut:                       # (one row's change is inside the bound of the sum of 264 rows: not the loss)
                assert got["rows"] >= 4.0, what
        for k in ("loss", "rows", "dsim"):
            assert _worst(ref[k].v.float().double(), ref[k]) <= 1.0
    me = L.ap_inputs(shape, me=True)
    ref, wrong = L.me_case(me), L.me_case(me, per_rows=True)
    got = {k: _worst(wrong[k], ref[k]) for k in ("loss", "dsim")}
    print(f"ME divided by rows [{shape}]: {got}")
    assert got["loss"] >= 4.0 and got["dsim"] >= 4.0
