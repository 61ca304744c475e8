"""G30: the VGGT teacher's camera head (vggt/heads/camera_head.py CameraHead, two tiny configurations) and the pose decoding
(vggt/utils/pose_enc.py pose_encoding_to_extri_intri) from the REFERENCE's own code, with the deterministic weights of tests/camera_layout.py
`fill_head` (empty_pose_tokens and the LayerScale gammas therefore non-zero), written to tests/golden/ (needs a checkout of the reference repository).
Camera-token inputs for (B, S) = (1, 2) and (2, 3); every iteration's encoding, extrinsics and intrinsics.  Before writing, the script checks that the
test's layout (tests/camera_layout.py) reproduces the reference, parameter layout included.  Usage: python tools/make_golden_g30.py <reference checkout>"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.abspath(sys.argv[1])
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), REF):
    sys.path.insert(0, p)
from camera_layout import CONFIGS, IMAGE_HW, SHAPES, CameraHeadLayout, decode_pose, fill_head, param_layout, seeded_tokens  # noqa: E402
from vggt.heads.camera_head import CameraHead  # noqa: E402
from vggt.utils.pose_enc import pose_encoding_to_extri_intri  # noqa: E402

torch.set_num_threads(1)          # one thread: the same summation order wherever the script runs
arrs, worst = {}, 0.0
with torch.no_grad():
    for cfg, kw in CONFIGS.items():
        ref = fill_head(CameraHead(**kw).eval())
        mirror = fill_head(CameraHeadLayout(**kw).eval())
        layout = param_layout(ref)
        assert param_layout(mirror) == layout, cfg
        assert float(ref.empty_pose_tokens.abs().min()) > 0 and float(ref.trunk[0].ls1.gamma.abs().min()) > 0
        arrs[f"{cfg}_param_layout"] = np.array(layout)
        for B, S in SHAPES:
            toks = seeded_tokens(cfg, B, S)
            want, got = ref(toks), mirror(toks)
            assert len(want) == len(got) == 4
            arrs[f"{cfg}_{B}x{S}_tokens"] = toks[-1].numpy()
            for it, (w, g) in enumerate(zip(want, got)):
                E, K = pose_encoding_to_extri_intri(w, IMAGE_HW)
                Eg, Kg = decode_pose(g, IMAGE_HW)
                for what, a, b in (("enc", w, g), ("extrinsic", E, Eg), ("intrinsic", K, Kg)):
                    assert bool(torch.isfinite(a).all()), (cfg, B, S, it, what)
                    e = float((a - b).abs().max()) / float(a.abs().max())
                    worst = max(worst, e)
                    assert e < 1e-5, (cfg, B, S, it, what, e)
                    arrs[f"{cfg}_{B}x{S}_{what}_{it}"] = a.numpy()
                assert float(w[..., 7:].min()) > 0.05 and float(w[..., 7:].max()) < 3.0, (cfg, B, S, it, w[..., 7:])
path = os.path.join(ROOT, "tests", "golden", "g30_camera_head.npz")
np.savez_compressed(path, **arrs)
print(f"wrote g30_camera_head.npz: {len(CONFIGS)} configurations x {len(SHAPES)} shapes x 4 iterations, {os.path.getsize(path)} bytes, layout vs reference "
      f"{worst:.2e} (relative)")
