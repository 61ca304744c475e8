"""G22: the VGGT teacher's aggregator (vggt/models/aggregator.py, tiny configuration) from the REFERENCE's own code, with the deterministic
weights of tests/test_teacher_runner_ref.py `fill_params`, written to tests/golden/ (needs a checkout of the reference repository).
Before writing, the script runs the teacher runner's hooks on the reference's Aggregator itself (QKCapture, _no_attention_maps) and checks
that the test's module layout reproduces the reference's outputs.  Usage: python tools/make_golden_g22.py <reference checkout>"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.abspath(sys.argv[1])
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), REF):
    sys.path.insert(0, p)
import gd_amd  # noqa: E402,F401
import gd_oracle as O  # noqa: E402
from gd_amd.teacher_runner import QKCapture, _no_attention_maps  # noqa: E402
from test_teacher_runner_ref import CFG, AggregatorLayout, fill_params  # noqa: E402
from vggt.models.aggregator import Aggregator  # noqa: E402

agg = Aggregator(img_size=CFG["img_size"], patch_size=CFG["patch_size"], embed_dim=CFG["embed_dim"], depth=CFG["depth"],
                 num_heads=CFG["num_heads"], num_register_tokens=CFG["num_register_tokens"], patch_embed="conv",
                 attn_indices=CFG["attn_indices"], temperature=CFG["temperature"]).eval()
fill_params(agg)
layout = ",".join(f"{n}:{'x'.join(map(str, p.shape))}" for n, p in sorted(agg.named_parameters()))
img = torch.rand(1, 2, 3, 56, 56, generator=torch.Generator().manual_seed(220))
with torch.no_grad():
    tokens, ps_idx, attn = agg(img)
    # the hooks on the reference's own modules
    sel = [agg.global_blocks[i].attn for i in agg.attn_indices]
    with QKCapture(sel) as cap, _no_attention_maps(sel):
        tokens2, _, placeholder = agg(img)
    assert placeholder.numel() == 1 and all(torch.equal(a, b) for a, b in zip(tokens, tokens2))
    qk = cap.pairs()
    maps = sum(O.cross_view_attention_maps(q.double(), k.double(), sel[0].scale, CFG["temperature"], prefix=5) for q, k in qk) / len(qk)
    err_hooks = float((maps - attn.mean(dim=1).double()).abs().max())
    assert err_hooks < 1e-6, err_hooks
    # the test's layout against the reference
    mirror = AggregatorLayout(**CFG).eval()
    assert ",".join(f"{n}:{'x'.join(map(str, p.shape))}" for n, p in sorted(mirror.named_parameters())) == layout
    fill_params(mirror)
    mt, mps, mattn = mirror(img)
    err_tok = max(float((a - b).abs().max()) for a, b in zip(mt, tokens))
    err_attn = float((mattn - attn).abs().max())
    assert mps == ps_idx and err_tok < 1e-4 * max(float(t.abs().max()) for t in tokens) and err_attn < 1e-6, (err_tok, err_attn)
arrs = {"img": img.numpy(), "attn_mean": attn.numpy(), "param_layout": np.array(layout)}
arrs.update({f"tokens_{i}": t.numpy() for i, t in enumerate(tokens)})
np.savez_compressed(os.path.join(ROOT, "tests", "golden", "g22_vggt_aggregator.npz"), **arrs)
print(f"wrote g22_vggt_aggregator.npz: {len(tokens)} token outputs {tuple(tokens[0].shape)}, attn_mean {tuple(attn.shape)}; hooks on the reference "
      f"{err_hooks:.2e}, layout vs reference: tokens {err_tok:.2e}, attn_mean {err_attn:.2e}")
