"""G28: the VGGT teacher's tracker from the REFERENCE's own code (vggt/heads/track_modules/base_track_predictor.py BaseTrackerPredictor on blocks.py
CorrBlock / EfficientUpdateFormer), the three cases of tests/tracker_layout.py CASES, with the deterministic weights of
tests/test_teacher_runner_ref.py `fill_params` and the two coordinate rows of `updateformer.flow_head` scaled by 0.05 (tracker_layout.condition_weights).
Before writing, the script checks that the test-owned module tree (tracker_layout.TrackerLayout) with the same fill reproduces all of it to 1e-4 of the
maximum, and that the reference's fp32 run stays within 1e-4 (relative to the largest coordinate) of its fp64 run on the final coordinates — the
conditioning check on the weights.  The fixture holds numeric arrays only: per case the correlation samples of iteration 1, the per-iteration
coordinates, `vis`, `conf`, and the parameter layout — no weights and no inputs (both are regenerated from seeds).
Build container only.  Usage: python tools/make_golden_g28.py"""
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
import vggt.heads.track_modules.base_track_predictor as BTP  # noqa: E402

import tracker_layout as TL  # noqa: E402
from test_teacher_runner_ref import fill_params  # noqa: E402


class TappedCorrBlock(BTP.CorrBlock):
    """Keeps what the first corr_sample call of an instance returned."""
    first = None

    def corr_sample(self, targets, coords):
        out = super().corr_sample(targets, coords)
        if TappedCorrBlock.first is None:
            TappedCorrBlock.first = out.detach().clone()
        return out


BTP.CorrBlock = TappedCorrBlock


def check(got, want, what):
    e, bound = float((got - want).abs().max()), 1e-4 * float(want.abs().max())
    assert got.shape == want.shape and e <= bound, (what, e, bound)
    return e / float(want.abs().max())


def reference(case):
    ref = BTP.BaseTrackerPredictor(stride=TL.STRIDE, corr_levels=TL.CASES[case]["levels"], corr_radius=TL.RADIUS, latent_dim=TL.LATENT,
                                   hidden_size=TL.HIDDEN, depth=TL.DEPTH).eval()
    fill_params(ref, seed=28)
    TL.condition_weights(ref)
    return ref


arrs, worst = {}, 0.0
for case in TL.CASES:
    ref, mirror = reference(case), TL.make_tracker(case)
    assert TL.param_layout(mirror) == TL.param_layout(ref), case
    q, fmaps = TL.seeded_inputs(case)
    with torch.no_grad():
        TappedCorrBlock.first = None
        coords, vis, conf = ref(q, fmaps, iters=TL.ITERS)
        corr = TappedCorrBlock.first
        taps = {}
        m_coords, m_vis, m_conf = mirror(q, fmaps, iters=TL.ITERS, taps=taps)
        coords64, _, _ = reference(case).double()(q.double(), fmaps.double(), iters=TL.ITERS)
    coords, m_coords = torch.stack(coords), torch.stack(m_coords)
    e64 = float((coords[-1] - coords64[-1]).abs().max()) / float(coords64[-1].abs().max())
    errs = [check(taps["corr"], corr, f"{case} corr"), check(m_coords, coords, f"{case} coords"), check(m_vis, vis, f"{case} vis"),
            check(m_conf, conf, f"{case} conf")]
    print(f"{case}: layout vs reference (rel. to max) corr {errs[0]:.1e} coords {errs[1]:.1e} vis {errs[2]:.1e} conf {errs[3]:.1e}; "
          f"the reference's fp32 run is {e64:.1e} from its fp64 run on the final coordinates")
    assert e64 <= 1e-4, (case, e64)
    worst = max(worst, *errs)
    arrs[f"{case}_corr"], arrs[f"{case}_coords"], arrs[f"{case}_vis"], arrs[f"{case}_conf"] = corr, coords, vis, conf
    arrs[f"{case}_param_layout"] = TL.param_layout(ref)

out = {k: (v.numpy() if torch.is_tensor(v) else np.array(v)) for k, v in arrs.items()}
path = os.path.join(ROOT, "tests", "golden", "g28_vggt_tracker.npz")
np.savez_compressed(path, **out)
print(f"wrote g28_vggt_tracker.npz ({os.path.getsize(path) / 1024:.0f} kB): cases {list(TL.CASES)}; layout vs reference, worst rel {worst:.2e}")
