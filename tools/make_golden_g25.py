"""G25: the MASt3R teacher's transformer blocks from the REFERENCE's own code (dust3r/croco/models/blocks.py Block / DecoderBlock with its
RoPE2D, AsymmetricCroCo3DStereo._decoder and .forward called unbound), tiny configuration (tests/croco_layout.py CFG), with the deterministic
weights of tests/test_teacher_runner_ref.py `fill_params`.  Before writing, the script checks that the test-owned module tree
(croco_layout.CrocoLayout) with the same fill reproduces all of it.  The fixture holds numeric arrays only: the input tokens and positions, the
encoder outputs, every `final_output` pair, `tgt_attn_map`, the head-mean score maps and the parameter layout — no weights.
Build container only.  Usage: python tools/make_golden_g25.py"""
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ref_import as R  # noqa: E402

R.install()
from dust3r.model import AsymmetricCroCo3DStereo  # noqa: E402
from models.blocks import Block, DecoderBlock  # noqa: E402
from models.pos_embed import RoPE2D  # noqa: E402

import croco_layout as CL  # noqa: E402
from test_teacher_runner_ref import fill_params  # noqa: E402

C = CL.CFG
norm = partial(nn.LayerNorm, eps=CL.LN_EPS)


class RefTeacher(nn.Module):
    """The reference's blocks under the attribute names of AsymmetricCroCo3DStereo; `_decoder` and `forward` are the reference's own functions."""
    _decoder = AsymmetricCroCo3DStereo._decoder
    forward = AsymmetricCroCo3DStereo.forward

    def __init__(self):
        super().__init__()
        rope = RoPE2D(100.0)
        self.enc_blocks = nn.ModuleList([Block(C["enc_dim"], C["enc_heads"], 4.0, qkv_bias=True, norm_layer=norm, rope=rope) for _ in range(C["enc_depth"])])
        self.enc_norm = norm(C["enc_dim"])
        self.decoder_embed = nn.Linear(C["enc_dim"], C["dec_dim"], bias=True)
        mk = lambda: DecoderBlock(C["dec_dim"], C["dec_heads"], mlp_ratio=4.0, qkv_bias=True, norm_layer=norm, norm_mem=True, rope=rope)
        self.dec_blocks = nn.ModuleList([mk() for _ in range(C["dec_depth"])])
        self.dec_blocks2 = nn.ModuleList([mk() for _ in range(C["dec_depth"])])
        self.dec_norm = norm(C["dec_dim"])
        self.reciprocity, self.temperature, self.count = C["reciprocity"], C["temperature"], 0
        self.feats = None

    # stubs for what `forward` calls around the decoder: the encoder hands out the features computed below, the heads return a placeholder
    def _encode_symmetrized(self, v1, v2):
        (f1, p1), (f2, p2) = self.feats
        return (None, None), (f1, f2), (p1, p2), (f1, f2)

    def _downstream_head(self, num, toks, shape):
        return {"pts3d": torch.zeros(1)}


ref = RefTeacher().eval()
fill_params(ref)
layout = CL.param_layout(ref)
x1, pos1, x2, pos2 = CL.seeded_inputs()
with torch.no_grad():
    enc = []
    for x, pos in ((x1, pos1), (x2, pos2)):
        for blk in ref.enc_blocks:
            x = blk(x, pos)
        enc.append(x)
    f1, f2 = ref.enc_norm(enc[0]), ref.enc_norm(enc[1])
    outs, maps1, maps2 = ref._decoder(f1, pos1, f2, pos2)
    ref.feats = ((f1, pos1), (f2, pos2))
    _, res2 = ref({"img": None}, {"img": None})
    tgt = res2["tgt_attn_map"]

    mirror = CL.CrocoLayout(**C).eval()
    assert CL.param_layout(mirror) == layout
    fill_params(mirror)
    menc = [mirror.encode_blocks(x1, pos1), mirror.encode_blocks(x2, pos2)]
    mouts, mtgt = mirror.target(mirror.enc_norm(menc[0]), pos1, mirror.enc_norm(menc[1]), pos2)
    _, mm1, mm2 = mirror._decoder(mirror.enc_norm(menc[0]), pos1, mirror.enc_norm(menc[1]), pos2)


def check(got, want, what):
    e, bound = float((got - want).abs().max()), 1e-4 * float(want.abs().max())
    assert e <= bound, (what, e, bound)
    return e


err_tok = max([check(a, b, f"enc {i}") for i, (a, b) in enumerate(zip(menc, enc))] +
              [check(a, b, f"view {v} output {i}") for v in range(2) for i, (a, b) in enumerate(zip(mouts[v], outs[v]))] +
              [check(a, b, f"maps {i}") for i, (a, b) in enumerate(zip(mm1 + mm2, maps1 + maps2))])
err_tgt = float((mtgt - tgt).abs().max())
assert err_tgt <= 1e-6, err_tgt
assert len(outs[0]) == C["dec_depth"] + 1 and tgt.shape == (CL.B, x1.shape[1], x2.shape[1])

arrs = {"x1": x1, "pos1": pos1, "x2": x2, "pos2": pos2, "enc_1": enc[0], "enc_2": enc[1], "tgt_attn_map": tgt}
for v in range(2):
    for i, t in enumerate(outs[v]):
        arrs[f"out{v + 1}_{i}"] = t
for l in range(C["dec_depth"]):
    arrs[f"camap1_{l}"] = maps1[l].mean(dim=1, keepdim=True)
    arrs[f"camap2_{l}"] = maps2[l].mean(dim=1, keepdim=True)
arrs = {k: v.numpy() for k, v in arrs.items()}
arrs["param_layout"] = np.array(layout)
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g25_mast3r_blocks.npz"), **arrs)
print(f"wrote g25_mast3r_blocks.npz: {len(outs[0])} output pairs, tgt_attn_map {tuple(tgt.shape)}; layout vs reference: tokens / maps {err_tok:.2e}, "
      f"tgt_attn_map {err_tgt:.2e}")
