"""G27: the MASt3R teacher's head from the REFERENCE's own code (mast3r/catmlp_dpt_head.py Cat_MLP_LocalFeatures_DPT_Pts3d with its postprocess,
built as mast3r_head_factory builds it), the tiny cases of tests/mast3r_head_layout.py CASES, with the deterministic weights of
tests/test_teacher_runner_ref.py `fill_params`.  Before writing, the script checks that the test-owned module tree (mast3r_head_layout.MASt3RHeadLayout)
with the same fill reproduces all of it, and that the reference's fp32 run agrees with its own fp64 run.  The fixture holds numeric arrays only: the
hooked input tokens, the image size, the map before the postprocess, the head's outputs and the parameter layouts — no weights.
Build container only.  Usage: python tools/make_golden_g27.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import ref_import as R  # noqa: E402

R.install()
from mast3r.catmlp_dpt_head import Cat_MLP_LocalFeatures_DPT_Pts3d, postprocess  # noqa: E402

import mast3r_head_layout as ML  # noqa: E402
from test_teacher_runner_ref import fill_params  # noqa: E402


def reference_head(cfg):
    """The head as mast3r_head_factory('catmlp+dpt', 'pts3d+desc<D>', net, has_conf) builds it, on a stand-in for the network's attributes."""
    net = types.SimpleNamespace(patch_embed=types.SimpleNamespace(patch_size=(ML.PATCH, ML.PATCH)), desc_mode=("norm",), two_confs=cfg["two_confs"],
                                desc_conf_mode=cfg["desc_conf_mode"], enc_embed_dim=ML.ENC, dec_embed_dim=ML.DEC, dec_depth=ML.DEC_DEPTH,
                                depth_mode=cfg["depth_mode"], conf_mode=cfg["conf_mode"])
    l2 = net.dec_depth
    head = Cat_MLP_LocalFeatures_DPT_Pts3d(net, local_feat_dim=cfg["local_feat_dim"], has_conf=cfg["has_conf"], num_channels=3 + cfg["has_conf"],
                                           feature_dim=ML.FEATURES, last_dim=ML.LAST_DIM, hooks_idx=[0, l2 * 2 // 4, l2 * 3 // 4, l2],
                                           dim_tokens=[ML.ENC, ML.DEC, ML.DEC, ML.DEC], postprocess=postprocess, depth_mode=net.depth_mode,
                                           conf_mode=net.conf_mode, head_type="regression").eval()
    fill_params(head)
    return head


def check(got, want, what):
    e, bound = float((got - want).abs().max()), 1e-4 * float(want.abs().max())
    assert got.shape == want.shape and e <= bound, (what, e, bound)
    return e


arrs, worst = {}, 0.0
for case, cfg in ML.CASES.items():
    ref = reference_head(cfg)
    mirror = ML.make_head(case)
    assert ML.param_layout(mirror) == ML.param_layout(ref), case
    assert list(ref.dpt.hooks) == ML.HOOKS
    fill_params(mirror)
    decout, (H, W) = ML.seeded_inputs(case)
    pre = {}
    ref.postprocess = lambda out, **kw: (pre.__setitem__("pre", out.detach().clone()), postprocess(out, **kw))[1]
    with torch.no_grad():
        want = ref(decout, (H, W))
        taps = {}
        got = mirror(decout, (H, W), taps=taps)
        want64 = reference_head(cfg).double()([t.double() for t in decout], (H, W))
    assert set(want) == set(got) == set(want64) == {"pts3d", "desc", "desc_conf"} | ({"conf"} if cfg["has_conf"] else set())
    for n in sorted(want):
        w, w64 = want[n], want64[n]
        e_64 = float((w - w64).abs().max()) / float(w64.abs().max())
        print(f"{case} {n}: {tuple(w.shape)}, max |.| {float(w.abs().max()):.3g}; the reference's fp32 run is {e_64:.1e} from its fp64 run (rel. to max)")
        assert w.dtype == torch.float32 and torch.isfinite(w).all() and e_64 <= 1e-5, (case, n)
        worst = max(worst, check(got[n], w, f"{case} {n}") / float(w.abs().max()))
        arrs[f"{case}_{n}"] = w
    worst = max(worst, check(taps["pre"], pre["pre"], f"{case} pre") / float(pre["pre"].abs().max()))
    arrs[f"{case}_pre"] = pre["pre"]
    for hook in ML.HOOKS:
        arrs[f"{case}_tokens_{hook}"] = decout[hook]
    arrs[f"{case}_image_hw"] = torch.tensor([H, W])
    arrs[f"{case}_param_layout"] = ML.param_layout(ref)

out = {k: (v.numpy() if torch.is_tensor(v) else np.array(v)) for k, v in arrs.items()}
path = os.path.join(ROOT, "tests", "golden", "g27_mast3r_head.npz")
np.savez_compressed(path, **out)
print(f"wrote g27_mast3r_head.npz ({os.path.getsize(path) / 1024:.0f} kB): cases {list(ML.CASES)}; layout vs reference, worst rel {worst:.2e}")
