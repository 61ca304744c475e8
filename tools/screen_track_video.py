"""Screen query seeds for tests/test_gpu_track.py::test_tapvid_video_metrics_end_to_end on the CPU: the oracle ViT's stride-8
features of the test's 4-frame video, the fp64 restatement of the tracker, and for every seed the point bound, the smallest
distance of a median from its threshold (the anchor frame whose median is the threshold excluded) and of a cosine from 0.6 / 0.7.
Prints the first seed whose margins exceed 10 x (2 x bound) and 10 x 1e-4."""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import gd_amd  # noqa: E402,F401
import gd_oracle as O  # noqa: E402
import track_ref64 as R64  # noqa: E402
from gd_amd.finetune import FinetuneGD
from gd_amd.synthetic import export_params
import test_gpu_track as TG
torch.manual_seed(0)
eng = FinetuneGD(r=4, backbone="vit_tiny_test", patch_size=16, img_size=128, variant="vggt", geometry="shared", dtype="f32",
                 lora_b_std=0.05, vit_kwargs=dict(init_values=1.0), teacher_patch=16).eval()
p, tr, refine, _, ocfg = export_params(eng)
ocfg = dict(ocfg, patch_stride=(8, 8))
H = W = 128; T = 4
frames = TG._video(T, H, W)
x = O.normalize_image(frames, ocfg["mean"], ocfg["std"])
_, last = O.vit_forward(x, p, ocfg, tr)
tok = O.final_norm(last, p, ocfg)[:, 1:]
og = tok.reshape(T, 15, 15, -1).permute(0, 3, 1, 2)
og = F.conv2d(og.double(), refine["weight"].double(), refine["bias"].double(), padding=1).permute(0, 2, 3, 1)
geom = (H, W, 16, 8, 15, 15, 15)
for seed in range(7, 80):
    g = torch.Generator().manual_seed(seed)
    worst_m, worst_c, bmax, ok = 1e9, 1e9, 0.0, True
    for f in (0, 2):
        q = (torch.rand(6, 2, generator=g) * (W - 40) + 20) * 2
        qq = torch.tensor([[0.5 * float(a), 0.5 * float(b), f] for a, b in q.tolist()], dtype=torch.float32)
        try:
            r = R64.infer(og, geom[:6], qq)
        except ValueError:
            ok = False; break
        bound = TG.check_rows(r["emb"].float().double().repeat(T, 1), torch.arange(T).repeat_interleave(6), og, geom, 35, "f32",
                              torch.float32, r["cells"].T.reshape(-1), r["tracks"].transpose(0, 1).reshape(-1, 2).float())
        bmax = max(bmax, bound)
        for n in range(6):
            med, th = r["meds"][n]
            A = r["anchors"][n]; tstar = set(int(a) for a in A if float(med[a]) == float(th))
            for t in range(T):
                if t not in tstar:
                    worst_m = min(worst_m, float((med[t] - th).abs()))
            worst_c = min(worst_c, float(torch.minimum((r["cos"][n] - 0.6).abs(), (r["cos"][n] - 0.7).abs()).min()))
    if ok:
        good = worst_m > 10 * 2 * bmax and worst_c > 10 * 1e-4
        print(seed, "bound", f"{bmax:.2e}", "med margin", f"{worst_m:.3e}", "cos margin", f"{worst_c:.3e}", "GOOD" if good else "", flush=True)
        if good:
            break
    else:
        print(seed, "empty anchors", flush=True)
