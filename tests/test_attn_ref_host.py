"""CPU: the fp64 restatement, the probe inputs and the derived bounds of tests/attn_ref64.py, before tests/test_gpu_attention_paths.py relies on
them.  (1) The restatement (backward as a function of the given o, lse) equals autograd of plain softmax attention.  (2) The probe inputs have
the properties the probes rest on.  (3) Every mutant of the restatement — a dropped / doubled key, a skipped tile or query, a live pad query, the
neighbouring head's k / v, the next row's lse — violates the per-element bound somewhere by a factor >= 4, at every size of the GPU grid and for
every operand type: the bounds are not vacuous.  GD_ATTN_MUTANTS=<file>: the smallest factor of every mutant is written there."""
import os

import pytest
import torch

import attn_ref64 as R

GRID = [1, 3, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 321, 383, 384, 385, 449, 513, 577, 705]
LONG = [3968, 4097]          # 16-bit types only (the DMA dK/dV forms on either side of the 4096 threshold)
B, H = 1, 2
FACTOR = 4.0
_MIN = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("GD_ATTN_MUTANTS")
    if path and _MIN:
        with open(path, "w") as f:
            for k in sorted(_MIN):
                f.write(f"{_MIN[k][0]:12.1f}  {k:40s} smallest at {_MIN[k][1]}\n")


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("N", [1, 3, 65, 193, 705])
def test_restatement_equals_autograd(N, family):
    qkv, dout = R.make_inputs(family, 2, N, 2, "bf16")
    q, k, v = R.heads(qkv, 2, N, 2)
    do = R.heads_o(dout, 2, N, 2)
    o, lse = R.fwd64(q, k, v)
    ao, alse, aq, ak, av = R.fwd_autograd64(q, k, v, do)
    assert _rel(o, ao) <= 1e-12 and float((lse - alse).abs().max()) <= 1e-12 * max(1.0, float(alse.abs().max()))
    dq, dk, dv = R.bwd64(q, k, v, o, lse, do)
    for got, ref in ((dq, aq), (dk, ak), (dv, av)):
        assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1e-30)
    # the bound functions restate the same operation in the exp2 domain
    fo, fl, bo, bl = R.fwd_bound(q, k, v, "bf16")
    gq, gk, gv, bq, bk, bv = R.bwd_bound(q, k, v, o, lse, do, "bf16")
    assert _rel(fo, o) <= 1e-12 and float((fl - lse).abs().max()) <= 1e-12 * max(1.0, float(lse.abs().max()))
    for got, ref in ((gq, dq), (gk, dk), (gv, dv)):
        assert float((got - ref).abs().max()) <= 1e-11 * max(float(ref.abs().max()), 1e-30)
    for b in (bo, bl, bq, bk, bv):
        assert bool(torch.isfinite(b).all()) and float(b.min()) >= 0.0


@pytest.mark.parametrize("N,kind", [(n, kd) for n in GRID + LONG for kd in ("bf16", "f16", "f32") if not (n in LONG and kd == "f32")])
def test_probe_input_conditions(N, kind):
    h = 1 if N in LONG else H
    qkv, dout = R.make_inputs("pair", B, N, h, kind)
    q, k, v = R.heads(qkv, B, N, h)
    _, lse = R.fwd64(q, k, v)
    p = torch.exp((q @ k.transpose(-1, -2)) * R.SCALE - lse[..., None])
    per_key, per_query = float(p.amax(-2).min()), float(p.amax(-1).min())
    print(f"pair N={N} {kind}: min over keys of max_i p = {per_key:.3f}, min over queries of max_j p = {per_query:.3f}")
    assert per_key >= 0.4 and per_query >= 0.2
    qkv, dout = R.make_inputs("uniform", B, N, h, kind)
    q, k, v = R.heads(qkv, B, N, h)
    do = R.heads_o(dout, B, N, h)
    assert float(q.abs().max()) == 0.0 and float(k.abs().max()) <= 3.0 and float(v.abs().max()) <= 3.0
    assert torch.equal(k, k.round()) and torch.equal(v, v.round())
    assert torch.equal(do.abs().sum(-1), torch.ones(B, h, N, dtype=torch.float64))      # one +-1 per row


def _note(mutant, family, factor, where):
    key = f"{mutant} / {family}"
    if factor < _MIN.get(key, (float("inf"), ""))[0]:
        _MIN[key] = (factor, where)


@pytest.mark.parametrize("N", GRID + LONG)
def test_every_mutant_exceeds_the_bound(N):
    kinds = ["bf16", "f16"] if N in LONG else list(R.KINDS)
    H = 1 if N in LONG else 2          # (one head at the long sizes, as on the GPU: the neighbouring-head mutant does not depend on N)
    muts = R.mutants(N, H)
    gaps = ([] if N % 64 and N > 1 else ["pad_query_live"] if N > 1 else ["lse_of_next_row"]) + (["neighbour_head_kv"] if H == 1 else [])
    assert [n for n, m in muts if m is None] == gaps
    cache = {}
    for kind in kinds:
        dt = R.KINDS[kind][0]
        if dt not in cache:                                     # f32 and x3 share their inputs: the reference and the mutants are computed once
            ent = {}
            for family in ("uniform", "pair"):
                qkv, dout = R.make_inputs(family, B, N, H, kind)
                q, k, v = R.heads(qkv, B, N, H)
                do = R.heads_o(dout, B, N, H)
                o, lse = R.fwd64(q, k, v)
                ref = (o, lse) + R.bwd64(q, k, v, o, lse, do)
                outs = {}
                for name, m in muts:
                    if m is not None:
                        mo, ml = R.fwd64(q, k, v, m)
                        outs[name] = (mo, ml) + R.bwd64(q, k, v, o, lse, do, m)
                ent[family] = (q, k, v, do, ref, outs)
            cache[dt] = ent
        for family in ("uniform", "pair"):
            q, k, v, do, ref, outs = cache[dt][family]
            o, lse = ref[0], ref[1]
            if family == "uniform":
                _, _, bo, bl = R.uniform_fwd(v, kind)
            else:
                _, _, bo, bl = R.fwd_bound(q, k, v, kind)
            bounds = (bo, bl) + R.bwd_bound(q, k, v, o, lse, do, kind)[3:]
            for name, m in muts:
                if m is None:
                    continue
                r = [R.ratio(g, t, b)[0] for g, t, b in zip(outs[name], ref, bounds)]      # o, lse, dq, dk, dv
                where = f"N={N} {kind}"
                if family == "uniform":
                    if m.key_w is not None:                     # the count mutants: through lse, against the fp32-accurate closed form
                        _note(name, family, r[1], where)
                        assert r[1] >= FACTOR, (name, family, where, r)
                    continue
                # the pair selector: through o or a gradient (one key alone, N = 1, has o = v whatever its multiplicity: dv shows it there)
                best = max(r[0], r[2], r[3], r[4])
                _note(name, family, best, where)
                assert best >= FACTOR, (name, family, where, r)
