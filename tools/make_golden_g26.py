"""G26: the VGGT teacher's dense-prediction head from the REFERENCE's own code (vggt/heads/dpt_head.py DPTHead with its activate_head and position
embedding), the three tiny cases of tests/dpt_layout.py CASES, with the deterministic weights of tests/test_teacher_runner_ref.py `fill_params`.
Before writing, the script checks that the test-owned module tree (dpt_layout.DPTLayout) with the same fill reproduces all of it, and that the
position embedding is separable into the two tables the fused head adds.  The fixture holds numeric arrays only: the input tokens, the image size,
the map before the activations (feature_only: the fused map before the last resampling), the head's outputs, the two position tables of case "a" at
image size, and the parameter layouts — no weights.
Build container only.  Usage: python tools/make_golden_g26.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ref_import as R  # noqa: E402

R.install()
from vggt.heads.dpt_head import DPTHead  # noqa: E402
from vggt.heads.utils import create_uv_grid, position_grid_to_embed  # noqa: E402

import dpt_layout as DL  # noqa: E402
from test_teacher_runner_ref import fill_params  # noqa: E402


def check(got, want, what):
    e, bound = float((got - want).abs().max()), 1e-4 * float(want.abs().max())
    assert got.shape == want.shape and e <= bound, (what, e, bound)
    return e


arrs, worst = {}, 0.0
for case, cfg in DL.CASES.items():
    kw = {k: v for k, v in cfg.items() if k != "grid"}
    ref = DPTHead(dim_in=DL.DIM_IN, patch_size=DL.PATCH, features=DL.FEATURES, out_channels=DL.OUT_CHANNELS, intermediate_layer_idx=DL.LAYER_IDX,
                  pos_embed=True, **kw).eval()
    fill_params(ref)
    mirror = DL.make_head(case)
    assert DL.param_layout(mirror) == DL.param_layout(ref)
    fill_params(mirror)
    toks, img = DL.seeded_inputs(case)
    pre = {}

    def keep_first(mod, a, out):            # (the first call is the unchunked run; a hook's return value would replace the output)
        pre.setdefault("pre", out.detach().clone())
    hook = (ref.scratch.output_conv1 if cfg["feature_only"] else ref.scratch.output_conv2).register_forward_hook(keep_first)
    with torch.no_grad():
        want = ref(toks, img, DL.PREFIX, frames_chunk_size=None)
        chunked = ref(toks, img, DL.PREFIX, frames_chunk_size=1)
        taps = {}
        got = mirror(toks, img, DL.PREFIX, taps=taps)
        ref64, t64 = DPTHead(dim_in=DL.DIM_IN, patch_size=DL.PATCH, features=DL.FEATURES, out_channels=DL.OUT_CHANNELS,
                             intermediate_layer_idx=DL.LAYER_IDX, pos_embed=True, **kw).eval(), [t.double() for t in toks]
        fill_params(ref64)
        want64 = ref64.double()(t64, img.double(), DL.PREFIX, frames_chunk_size=None)
    hook.remove()
    want, chunked, got, want64 = [(t,) if torch.is_tensor(t) else tuple(t) for t in (want, chunked, got, want64)]
    names = ("features",) if cfg["feature_only"] else ("preds", "conf")
    for n, w, c, g, w64 in zip(names, want, chunked, got, want64):
        e_chunk, e_64 = float((w - c).abs().max()) / float(w.abs().max()), float((w - w64).abs().max()) / float(w64.abs().max())
        print(f"{case} {n}: the reference's frame chunking moves it by {e_chunk:.1e}, its fp32 run is {e_64:.1e} from its fp64 run (rel. to max)")
        assert e_chunk <= 1e-5 and e_64 <= 1e-5, (case, n)
        worst = max(worst, check(g, w, f"{case} {n}") / float(w.abs().max()))
        arrs[f"{case}_{n}"] = w
    worst = max(worst, check(taps["pre"], pre["pre"], f"{case} pre") / float(pre["pre"].abs().max()))
    arrs[f"{case}_pre"] = pre["pre"]
    for i, t in enumerate(toks):
        arrs[f"{case}_tokens_{i}"] = t
    arrs[f"{case}_image_hw"] = torch.tensor(img.shape[-2:])
    arrs[f"{case}_param_layout"] = DL.param_layout(ref)

# the position embedding of case "a" at image size: separable, and equal to the two tables
gh, gw = DL.CASES["a"]["grid"]
H, W, C = gh * DL.PATCH, gw * DL.PATCH, DL.FEATURES // 2
emb = position_grid_to_embed(create_uv_grid(W, H, aspect_ratio=W / H, dtype=torch.float32), C) * 0.1          # [H, W, C]
px, py = emb[0, :, :C // 2].clone(), emb[:, 0, C // 2:].clone()
assert torch.equal(emb[..., :C // 2], px[None].expand(H, W, C // 2)) and torch.equal(emb[..., C // 2:], py[:, None].expand(H, W, C // 2))
mpx, mpy = DL.pos_tables(W, H, C, W / H)
assert float((mpx - px).abs().max()) <= 1.5e-8 and float((mpy - py).abs().max()) <= 1.5e-8
arrs["a_px"], arrs["a_py"] = px, py

out = {k: (v.numpy() if torch.is_tensor(v) else np.array(v)) for k, v in arrs.items()}
path = os.path.join(ROOT, "tests", "golden", "g26_dpt_head.npz")
np.savez_compressed(path, **out)
print(f"wrote g26_dpt_head.npz ({os.path.getsize(path) / 1024:.0f} kB): cases {list(DL.CASES)}; layout vs reference, worst rel {worst:.2e}")
