"""Host: the fp64 restatement of csrc/rows.hip (tests/rows_ref64.py).  On every case of the tables the GPU tests use, (a) the same expression
evaluated in fp32 on the CPU stays inside the derived bound — the bound is not tighter than fp32 arithmetic itself, whatever the summation order —
and (b) each deliberate mistake (rows_ref64.MUTANTS) breaks the bound by a factor of at least 4: a kernel with that mistake cannot pass."""
import pytest
import torch

import rows_ref64 as R

LIN_IDS = [f"{i}-M{c['M']}-K{c['K']}-N{c['N']}-{c['wt']}" for i, c in enumerate(R.LINEAR_CASES)]


def worst(got, want, bound):
    return float(((got.double() - want.double()).abs() / bound).max())


def lin(c, mutant=None, dtype=torch.float64):
    i = R.linear_inputs(c)
    return R.linear64(i["x"], i["w"], i["bias"], i["residual"], i["gamma"], c["silu"], c["gelu"], mutant=mutant, dtype=dtype)


@pytest.mark.parametrize("c", R.LINEAR_CASES, ids=LIN_IDS)
def test_linear_fp32_evaluation_is_inside_the_bound(c):
    want, bound = lin(c)
    got, _ = lin(c, dtype=torch.float32)
    r = worst(got, want, bound)
    print(f"linear fp32 CPU vs fp64: worst err / bound {r:.3f}")
    assert got.dtype == torch.float32 and r <= 1.0


@pytest.mark.parametrize("c", R.LINEAR_CASES, ids=LIN_IDS)
def test_linear_mutants_break_the_bound(c):
    want, bound = lin(c)
    applies = {"last_k_chunk_dropped": True, "neighbour_bias": c["bias"], "gamma_on_residual": c["residual"] and c["gamma"], "silu_omitted": c["silu"]}
    for m, on in applies.items():
        if on:
            r = worst(lin(c, m)[0], want, bound)
            print(f"linear mutant {m}: worst err / bound {r:.1f}")
            assert r >= 4.0, m


def test_every_prologue_and_epilogue_of_the_head_and_every_mutant_is_in_the_tables():
    forms = {(c["silu"], c["gelu"], c["residual"], c["gamma"]) for c in R.LINEAR_CASES}
    # embed / qkv / pose fc2; modulation; fc1; proj / fc2 with LayerScale; the same with ls = Identity
    assert {(False, False, False, False), (True, False, False, False), (False, True, False, False), (False, False, True, True), (False, False, True, False)} <= forms
    assert {c["M"] for c in R.LINEAR_CASES} == {1, 2, 3, 8} and {c["wt"] for c in R.LINEAR_CASES} == {"f32", "bf16"}
    assert {4, 12, 252, 256, 260, 2048, 8192} <= {c["K"] for c in R.LINEAR_CASES} and {1, 9, 31, 32, 33, 2048} <= {c["N"] for c in R.LINEAR_CASES}
    assert all(c["M"] * c["K"] <= 16384 for c in R.LINEAR_CASES)
    assert len(R.MUTANTS) == 9


@pytest.mark.parametrize("B,S,H,hd", R.ATTENTION_CASES)
def test_attention_bound_and_mutants(B, S, H, hd):
    for huge in (None, B - 1):
        qkv = R.attention_inputs(B, S, H, hd, pad=4, huge_entry=huge)
        want, bound = R.attention64(qkv, B, S, H, hd)
        got, _ = R.attention64(qkv, B, S, H, hd, dtype=torch.float32)
        r = worst(got, want, bound)
        print(f"attention fp32 CPU vs fp64 (huge entry {huge}): worst err / bound {r:.3f}")
        assert r <= 1.0
        for m, on in (("attention_across_entries", B > 1), ("dropped_key", S > 1)):
            if on:
                rm = worst(R.attention64(qkv, B, S, H, hd, mutant=m)[0], want, bound)
                print(f"attention mutant {m}: {rm:.1f}")
                assert rm >= 4.0, m


def test_attention_is_the_modules_forward_between_qkv_and_proj():
    """camera_layout._Attention with identity projections is the restatement."""
    import camera_layout as CL
    B, S, H, hd = 2, 3, 4, 16
    at = CL._Attention(H * hd, H).double()
    x = torch.randn(B, S, H * hd, generator=R.gen(5), dtype=torch.float64)
    with torch.no_grad():
        qkv = at.qkv(x).reshape(B * S, -1)
        at.proj.weight.copy_(torch.eye(H * hd, dtype=torch.float64))
        at.proj.bias.zero_()
        want = at(x).reshape(B * S, -1)
    got, _ = R.attention64(qkv, B, S, H, hd)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())


@pytest.mark.parametrize("M,D", R.ADALN_CASES)
def test_adaln_bound_and_mutant(M, D):
    x, mod = R.adaln_inputs(M, D)
    want, bound = R.adaln64(x, mod)
    got, _ = R.adaln64(x, mod, dtype=torch.float32)
    r = worst(got, want, bound)
    rm = worst(R.adaln64(x, mod, mutant="gate_scale_swapped")[0], want, bound)
    print(f"adaLN fp32 CPU vs fp64: worst err / bound {r:.3f}; gate and scale swapped: {rm:.1f}")
    assert r <= 1.0 and rm >= 4.0
    ln = torch.nn.LayerNorm(D, elementwise_affine=False, eps=1e-6).double()
    sh, sc, g = mod.double().chunk(3, dim=-1)
    assert float((want - (g * (ln(x.double()) * (1 + sc) + sh) + x.double())).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("first,acts", R.POSE_CASES)
def test_pose_bound_and_mutants(first, acts):
    delta, raw = R.pose_inputs(first, acts)
    want = R.pose64(delta, raw, first, acts, R.POSE_HW)
    got = R.pose64(delta, raw, first, acts, R.POSE_HW, dtype=torch.float32)
    r = R.pose_ratio(got, want)
    print(f"pose fp32 CPU vs fp64: worst err / bound {r:.3f}")
    assert r <= 1.0 and not bool(torch.isnan(got["intrinsic"]).any())
    fov = want["enc"][:, 7:9]
    if acts[2] == "relu":
        assert float(fov[0, 0]) == 0.0 and bool(torch.isposinf(want["intrinsic"][0, 1, 1])) and bool(torch.isposinf(got["intrinsic"][0, 1, 1]))
        fov = fov[1:]
    assert float(fov.min()) >= R.FOV_RANGE[0] and float(fov.max()) <= R.FOV_RANGE[1]
    for m, on in (("activated_fed_back", not first), ("scalar_first_quaternion", True)):
        if on:
            rm = R.pose_ratio(R.pose64(delta, raw, first, acts, R.POSE_HW, mutant=m), want)
            print(f"pose mutant {m}: {rm:.1f}")
            assert rm >= 4.0, m


def test_pose_restatement_is_the_layouts_activation_and_decoding():
    import camera_layout as CL
    delta, raw = R.pose_inputs(False, ("inv_log", "linear", "relu"), seed=3)
    want = R.pose64(delta, raw, False, ("inv_log", "linear", "relu"), R.POSE_HW)
    head = CL.CameraHeadLayout(dim_in=8, trunk_depth=1, num_heads=1, trans_act="inv_log")
    enc = head.activate(raw[:, :9].double() + delta.double())
    E, K = CL.decode_pose(enc[1:], R.POSE_HW)
    assert torch.equal(enc, want["enc"])
    assert float((E - want["extrinsic"][1:]).abs().max()) <= 1e-13 and float((K - want["intrinsic"][1:]).abs().max()) <= 1e-10
