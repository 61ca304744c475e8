"""Correspondence-evaluation timings on one GPU (not the training benchmark: bench.py stays the yardstick of the step).

  python3 tools/bench_match.py [--out FILE] [--iters 5] [--warm 2]

1. The OnePose++-sized matcher, M = 16384 query descriptors x N = 120000 templates x D = 768, both directions, in f16 and f32:
   gd_match_argmax (one pass, argmax fused) against the reference's form on torch (src/evaluate_timm.py:166-179: two chunked
   `d @ templates.T` + argmax, one per direction, chunks of 2.5e8 scores).  TFLOP/s counts ONE similarity GEMM, 2 M N D; the
   fraction is of bench.PEAK_TFLOPS (fp16 MFMA for f16, fp32 MFMA for f32).
2. One semantic-transfer pair at 640^2 (40 x 40 tokens, D = 768, 20 keypoints): gd_amd.evaluate.transfer_keypoints_from_tokens
   against the reference's materialising form (interpolate to 625^2 -> edge pad -> einsum -> argmax, src/evaluate_timm.py:531-547):
   time and peak allocated memory.
The torch forms are comparisons inside this tool only.  Prints one JSON object (also written to --out)."""
import argparse
import hashlib
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gd_amd  # noqa: E402,F401
from gd_amd import _lib, ops  # noqa: E402
from gd_amd import evaluate as E  # noqa: E402
from bench import PEAK_TFLOPS  # noqa: E402


def timed(fn, warm, iters):
    """ms per call: device events around `iters` calls after `warm` warm-up calls; also the spread over single-call timings."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    singles = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        singles.append(e0.elapsed_time(e1))
    singles.sort()
    return {"median_ms": round(singles[len(singles) // 2], 3), "min_ms": round(singles[0], 3), "max_ms": round(singles[-1], 3)}


def torch_nn_both(desc, temp):
    """src/evaluate_timm.py:166-179 restated on torch tensors (comparison only)."""
    nbr1 = torch.cat([(d @ temp.T).argmax(-1) for d in torch.split(desc, (25000 * 10000 - 1) // temp.shape[0] + 1)], 0)
    nbr2 = torch.cat([(d @ desc.T).argmax(-1) for d in torch.split(temp, (25000 * 10000 - 1) // desc.shape[0] + 1)], 0)
    return nbr1, nbr2


def torch_transfer(tok1, tok2, kps, img=640, p=16):
    """src/evaluate_timm.py:531-547 restated (comparison only): the 640^2 x D field is materialised."""
    gh = 1 + (img - p) // p
    d1 = tok1.reshape(1, gh, gh, -1).permute(0, 3, 1, 2)
    d2 = tok2.reshape(1, gh, gh, -1).permute(0, 3, 1, 2)
    ds = ((img - p) // p) * p + 1
    d2 = F.interpolate(d2, size=(ds, ds), mode="bilinear", align_corners=True)
    d2 = F.pad(d2, (p // 2, img - ds - p // 2, p // 2, img - ds - p // 2), mode="replicate")
    g = E.keypoint_grid_coords(kps[None, :, :2], img, img)[:, None]
    q = F.normalize(F.grid_sample(d1, g, align_corners=True, padding_mode="border")[:, :, 0], dim=1)       # [1, D, K]
    sim = torch.einsum("nfk,nif->nki", q, d2.permute(0, 2, 3, 1).reshape(1, img * img, -1))[0]
    idx = sim.argmax(dim=1)
    return torch.stack([idx % img, idx // img], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--M", type=int, default=16384)
    ap.add_argument("--N", type=int, default=120000)
    ap.add_argument("--D", type=int, default=768)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"library_sha256_16": hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16], "device": torch.cuda.get_device_name(0)}

    M, N, D = a.M, a.N, a.D
    desc = F.normalize(torch.randn(M, D, device=dev), dim=1)
    temp = F.normalize(torch.randn(N, D, device=dev), dim=1)
    flop = 2.0 * M * N * D
    mres = {"M": M, "N": N, "D": D, "flop_one_gemm": flop}
    for prec in ("f16", "f32"):
        peak = PEAK_TFLOPS["tf32h" if prec == "f16" else "f32"]
        ours = timed(lambda: ops.match_argmax(desc, temp, precision=prec, want_mutual=True), a.warm, a.iters)
        ent = {"ours_call": ours, "ours_call_tflops": round(flop / ours["median_ms"] * 1e-9, 1)}
        if prec == "f16":       # the kernel alone, on operands already in fp16 (the call above includes the scaled casts)
            d16, t16 = desc.half(), temp.half()
            k = timed(lambda: ops.match_argmax(d16, t16, precision="f16", want_mutual=True), a.warm, a.iters)
            ent["ours_kernel_only"] = k
            ent["ours_kernel_tflops"] = round(flop / k["median_ms"] * 1e-9, 1)
            ent["ours_kernel_frac_of_peak"] = round(flop / k["median_ms"] * 1e-9 / peak, 4)
            dt, tt = d16, t16
        else:
            ent["ours_call_frac_of_peak"] = round(flop / ours["median_ms"] * 1e-9 / peak, 4)
            dt, tt = desc, temp
        ref = timed(lambda: torch_nn_both(dt, tt), a.warm, a.iters)
        ent["torch_two_pass"] = ref
        ent["speedup_vs_torch"] = round(ref["median_ms"] / ours["median_ms"], 2)
        r = ops.match_argmax(desc, temp, precision=prec)
        n1, n2 = torch_nn_both(dt, tt)
        ent["agree_with_torch_rows"] = round(float((r.row_idx == n1).float().mean()), 6)
        ent["agree_with_torch_cols"] = round(float((r.col_idx == n2).float().mean()), 6)
        ent["peak_tflops"] = peak
        mres[prec] = ent
        torch.cuda.empty_cache()
    res["matcher"] = mres
    del desc, temp
    torch.cuda.empty_cache()

    img, p, Dt, K = 640, 16, 768, 20
    gh = 1 + (img - p) // p
    tok1 = torch.randn(gh * gh, Dt, device=dev)
    tok2 = torch.randn(gh * gh, Dt, device=dev)
    kps = torch.randint(0, img, (K, 2), device=dev).float()
    tres = {}
    for name, fn in (("ours", lambda: E.transfer_keypoints_from_tokens(tok1, tok2, kps, img, p, p)),
                     ("torch_materialised", lambda: torch_transfer(tok1, tok2, kps, img, p))):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        ent = timed(fn, a.warm, a.iters)
        ent["peak_extra_bytes"] = torch.cuda.max_memory_allocated() - base
        tres[name] = ent
    xo, xt = E.transfer_keypoints_from_tokens(tok1, tok2, kps, img, p, p), torch_transfer(tok1, tok2, kps, img, p)
    tres["agree_with_torch"] = round(float((xo == xt).all(1).float().mean()), 4)
    tres["speedup_vs_torch"] = round(tres["torch_materialised"]["median_ms"] / tres["ours"]["median_ms"], 2)
    res["semantic_transfer_pair_640"] = tres
    txt = json.dumps(res)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
