"""G29: the VGGT teacher's DINOv2 patch embedder (vggt/layers/vision_transformer.py, tiny configuration) from the REFERENCE's own code, with the
deterministic weights of tests/test_teacher_runner_ref.py `fill_params`, written to tests/golden/ (needs a checkout of the reference repository).
Four image sizes: the position table's own grid, two non-square ones (the bicubic antialias resampling) and a square resampled one.  The same script
builds the reference's Aggregator around `dinov2_vits14_reg` and, before writing, checks that the test's layouts (tests/dino_layout.py) reproduce the
reference's outputs.  Usage: python tools/make_golden_g29.py <reference checkout>"""
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.abspath(sys.argv[1])
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), REF):
    sys.path.insert(0, p)
from dino_layout import AGG_CFG, AGG_DINO, DINO_CFG, DINO_SIZES, DinoAggregatorLayout, DinoLayout, param_layout  # noqa: E402
from test_teacher_runner_ref import fill_params  # noqa: E402
from vggt.layers import MemEffAttention, NestedTensorBlock  # noqa: E402
from vggt.layers.vision_transformer import DinoVisionTransformer  # noqa: E402
from vggt.models.aggregator import Aggregator  # noqa: E402

torch.set_num_threads(1)          # one thread: the same summation order wherever the script runs
ref = DinoVisionTransformer(**DINO_CFG, interpolate_antialias=True, interpolate_offset=0.0, init_values=1.0, block_chunks=0,
                            block_fn=partial(NestedTensorBlock, attn_class=MemEffAttention)).eval()
fill_params(ref)
layout = param_layout(ref)
mirror = DinoLayout(**DINO_CFG).eval()
assert param_layout(mirror) == layout
fill_params(mirror)
arrs, worst = {"param_layout": np.array(layout)}, 0.0
with torch.no_grad():
    for i, (H, W) in enumerate(DINO_SIZES):
        img = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(290 + i))          # an already normalised image
        out, got = ref(img), mirror(img)
        for k in ("x_prenorm", "x_norm_patchtokens"):
            e = float((out[k] - got[k]).abs().max()) / float(out[k].abs().max())
            worst = max(worst, e)
            assert e < 1e-6, (H, W, k, e)
            arrs[f"{k}_{H}x{W}"] = out[k].numpy()
        arrs[f"img_{H}x{W}"] = img.numpy()
    # the reference's Aggregator around the DINO embedder, on a non-square pair
    agg = Aggregator(img_size=AGG_CFG["img_size"], embed_dim=AGG_CFG["embed_dim"], depth=AGG_CFG["depth"], num_heads=AGG_CFG["num_heads"],
                     patch_embed="dinov2_vits14_reg").eval()
    fill_params(agg)
    agg_layout = param_layout(agg)
    amirror = DinoAggregatorLayout(**AGG_CFG, dino_depth=AGG_DINO["depth"], dino_heads=AGG_DINO["num_heads"]).eval()
    assert param_layout(amirror) == agg_layout
    fill_params(amirror)
    aimg = torch.rand(1, 2, 3, 42, 70, generator=torch.Generator().manual_seed(299))
    tokens, ps_idx, _ = agg(aimg)
    mt, mps, _ = amirror(aimg)
    err_tok = max(float((a - b).abs().max()) for a, b in zip(mt, tokens))
    assert mps == ps_idx and len(mt) == len(tokens) and err_tok < 1e-4 * max(float(t.abs().max()) for t in tokens), err_tok
arrs.update({"agg_img": aimg.numpy(), "agg_ps_idx": np.array(ps_idx)})
arrs.update({f"agg_tokens_{i}": t.numpy() for i, t in enumerate(tokens)})
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g29_dino_embed.npz"), **arrs)
print(f"wrote g29_dino_embed.npz: {len(DINO_SIZES)} image sizes, layout vs reference {worst:.2e} (relative); aggregator: {len(tokens)} token outputs "
      f"{tuple(tokens[0].shape)}, ps_idx {ps_idx}, layout vs reference {err_tok:.2e}")
