"""Correspondence evaluation of a fine-tuned backbone: the three methods the reference's EvaluationCallback runs every 10 epochs
(src/evaluate_timm.py:591-730) — semantic keypoint transfer (:461-588), the OnePose++ descriptor matching (:140-179) and TAP-Vid
tracking (:234-348) — with the features on the HIP forward, the matching on gd_match_argmax / gd_transfer_argmax and the tracker
head on gd_track_points.  Everything runs under torch.no_grad(); nothing here touches the training step's caches
(FinetuneGD._forward / _kp_pair are keyed by data_ptr and belong to the step).  Dataset readers, image decoding and resizing, the
random template subsample and PnP (cv2) stay with the caller.

The reference's own quirks are kept, because the numbers it reports depend on them:
  - the query keypoints of the transfer are sampled with interpolate_features' DEFAULT mapping (patch 14, stride 14) on the
    patch-16 token grid (:542);
  - the target field is the grid upsampled to ds = ((img - p) // s) * s + 1 and edge-padded by p // 2 (:531-538);
  - OnePose++ descriptors are sampled at patch 16 and divided by (norm + 1e-9) (:160-163).
The hard-coded 16 is generalised to the model's patch and stride (equal to the reference's at p = s = 16)."""
import torch

from . import ops
from ._lib import GdHipError


# ----------------------------------------------------------------------------------------------------------------- geometry (host)
def token_grid(img_h, img_w, patch, stride):
    """Token grid of a patch-`patch` / stride-`stride` embedding of an img_h x img_w image: (1 + (img_h - p) // s, 1 + (img_w - p) // s)."""
    if patch <= 0 or stride <= 0 or img_h < patch or img_w < patch:
        raise GdHipError(f"no token grid for image {img_h}x{img_w} at patch {patch}, stride {stride}")
    return 1 + (img_h - patch) // stride, 1 + (img_w - patch) // stride


def transfer_geometry(img_h, img_w, patch, stride):
    """The field of src/evaluate_timm.py:531-538 generalised: -> dict(gh, gw, ds_h, ds_w, top, left, bottom, right).  The grid is
    upsampled to ds = ((img - p) // s) * s + 1 and edge-padded by p // 2 on the top / left and img - ds - p // 2 on the bottom / right."""
    gh, gw = token_grid(img_h, img_w, patch, stride)
    ds_h, ds_w = ((img_h - patch) // stride) * stride + 1, ((img_w - patch) // stride) * stride + 1
    return {"gh": gh, "gw": gw, "ds_h": ds_h, "ds_w": ds_w, "top": patch // 2, "left": patch // 2,
            "bottom": img_h - ds_h - patch // 2, "right": img_w - ds_w - patch // 2}


def keypoint_grid_coords(pts, h, w, patch_size=14, stride=14):
    """interpolate_features' pixel -> grid_sample mapping (utils/functions.py:56-65), in fp32 as the reference computes it:
    pts [..., 2] (x, y) -> [..., 2] in [-1, 1] at the patch centres (7 -> -1 and 623 -> +1 at 640 with the default patch 14)."""
    last_h = ((h - patch_size) // stride) * stride + patch_size / 2
    last_w = ((w - patch_size) // stride) * stride + patch_size / 2
    a = torch.tensor([2 / (last_w - patch_size / 2), 2 / (last_h - patch_size / 2)], dtype=torch.float32, device=pts.device)
    b = torch.tensor([1 - last_w * 2 / (last_w - patch_size / 2), 1 - last_h * 2 / (last_h - patch_size / 2)], dtype=torch.float32,
                     device=pts.device)
    return a * pts.float() + b


def pck(pred_xy, gt_xy, img_size, alphas=(0.10, 0.05, 0.15)):
    """PCK of src/evaluate_timm.py:557-566 on the visible keypoints: fraction with ||pred - gt|| < alpha * img_size, per alpha
    -> fp32 [len(alphas)].  pred_xy int or float [N, 2], gt_xy float [N, 2] (host tensors)."""
    gt = gt_xy.cpu()
    err = (pred_xy.cpu() - gt).norm(dim=-1)
    thr = torch.tensor(alphas) * img_size
    return (err[None, :] < thr[:, None]).sum(dim=-1) / len(gt)


# ----------------------------------------------------------------------------------------------------------------- features
def _backbone(module):
    m = module.model if hasattr(module, "model") else module
    P = m.patch_embed.patch_size[0]
    st = m.patch_embed.proj.stride
    st = (st, st) if isinstance(st, int) else tuple(int(v) for v in st)
    if st[0] != st[1]:
        raise GdHipError(f"correspondence evaluation needs one patch stride, got {st}")
    return m, P, st[0]


def _image(img):
    img = img if img.dim() == 4 else img[None]
    if not (img.is_cuda and img.dtype == torch.float32 and img.shape[1] == 3):
        raise GdHipError("evaluation images are CUDA fp32 [3, H, W] (or [B, 3, H, W]) in [0, 1]")
    return img


def token_maps(module, img):
    """module.model.forward_features on the HIP path, then refine_conv on the whole token grid when the module has one
    (vit.conv3x3_tokens) -> (grid [B, gh * pitch, D] token-major without prefix tokens, gh, gw, pitch)."""
    from .vit import conv3x3_tokens
    m, P, st = _backbone(module)
    img = _image(img)
    H, W = img.shape[-2:]
    gh, gw = token_grid(H, W, P, st)
    with torch.no_grad():
        x = m.forward_features(img)
        prefix = m.num_prefix_tokens
        if x.shape[1] - prefix != gh * gw:
            raise GdHipError(f"the model returned {x.shape[1] - prefix} patch tokens for a {H}x{W} image; patch {P} / stride {st} "
                             f"give a {gh}x{gw} grid")
        rc = getattr(module, "refine_conv", None)
        if rc is not None:
            fmap, pitch = conv3x3_tokens(x, rc.weight, rc.bias, gh, gw)
            return fmap, gh, gw, pitch
        return x[:, prefix:], gh, gw, gw


def _sample(grid, pts, gh, gw, pitch, h, w, patch_size, stride):
    """interpolate_features(normalize=False) on a token-major grid [B, gh * pitch, D] -> [B, N, D] fp32."""
    from .vit import kp_gather
    return kp_gather([grid.contiguous()], pts.float().contiguous(), gh, gw, 1.0, 1.0, h, w, patch_size, stride=stride, pitch=pitch)


def _normalize(x, normalize):
    if normalize is False or normalize is None:
        return x
    if normalize is True:
        return ops.l2_normalize(x.contiguous())                              # F.normalize: x / max(||x||, 1e-12)
    if normalize == "onepose":
        return ops.l2_normalize(x.contiguous(), eps=1e-9)                    # x / (||x|| + 1e-9): the same rows wherever ||x|| >> 1e-9
    raise GdHipError(f"normalize must be True, False or 'onepose', not {normalize!r}")


def descriptors_at(module, img, pts, *, patch_size, stride, normalize):
    """Descriptors of `module` at pixel positions: forward_features (prefix tokens dropped) -> refine_conv on the whole grid if
    the module has one -> interpolate_features(pts, h, w = the image's, patch_size, stride).  img [3, H, W] or [B, 3, H, W]
    in [0, 1]; pts [N, 2] or [B, N, 2] (x, y); normalize True (F.normalize), False, or "onepose" (/(norm + 1e-9)).
    -> [N, D] (or [B, N, D]) fp32."""
    with torch.no_grad():
        single = pts.dim() == 2
        img = _image(img)
        grid, gh, gw, pitch = token_maps(module, img)
        p = pts[None] if single else pts
        if p.shape[0] != grid.shape[0]:
            p = p.expand(grid.shape[0], -1, -1)
        out = _normalize(_sample(grid, p.to(grid.device), gh, gw, pitch, img.shape[-2], img.shape[-1], patch_size, stride), normalize)
        return out[0] if single else out


# ----------------------------------------------------------------------------------------------------------------- OnePose++ matching
def mutual_nearest_neighbours(desc, templates, precision="f16"):
    """The matching block of src/evaluate_timm.py:166-179 from ONE pass of gd_match_argmax: desc [M, D], templates [N, D] ->
    (nbr1 [M] int64 = argmax_j desc_i . t_j, nbr2 [N] int64 = argmax_i desc_i . t_j, mutual [M] bool = nbr2[nbr1] == arange(M)).
    precision "f16" (the reference's TF32 class, fp16 operands under per-tensor power-of-two scales) or "f32" (exact)."""
    with torch.no_grad():
        r = ops.match_argmax(desc, templates, both=True, precision=precision, want_mutual=True)
        return r.row_idx, r.col_idx, r.mutual


# ----------------------------------------------------------------------------------------------------------------- semantic transfer
def _img_hw(img_size):
    return (int(img_size), int(img_size)) if isinstance(img_size, int) else tuple(int(v) for v in img_size)


def transfer_keypoints_from_tokens(tok1, tok2, kps1, img_size=640, patch_size=16, stride=16, query_patch=14, query_stride=14,
                                   pitch=None):
    """kps_1_to_2 of src/evaluate_timm.py:539-547 from the two views' token maps: tok1, tok2 [gh, gw, D] or token-major
    [gh * pitch, D] (after refine_conv when the model has one), gh x gw = 1 + (img - patch) // stride; kps1 [K, >= 2] (x, y, ...).
    The queries are interpolate_features(tok1, kps1, img, img, normalize=True) with the reference's default query mapping
    (query_patch = query_stride = 14); the target field is never materialised: S = q . tok2 on the grid, then the argmax over
    the upsampled, padded S (gd_transfer_argmax).  -> [K, 2] int64 (x, y)."""
    img_h, img_w = _img_hw(img_size)
    gh, gw = token_grid(img_h, img_w, patch_size, stride)
    pitch = gw if pitch is None else int(pitch)
    with torch.no_grad():
        toks = []
        for t in (tok1, tok2):
            t = t.reshape(-1, t.shape[-1])
            if t.shape[0] != gh * pitch:
                raise GdHipError(f"token map of {t.shape[0]} rows; image {img_h}x{img_w} at patch {patch_size}, stride {stride} needs "
                                 f"{gh}x{gw} (pitch {pitch})")
            if not t.is_cuda:
                raise GdHipError("token maps must be CUDA tensors")
            toks.append(t.contiguous() if t.dtype == torch.float32 else ops.cast(t, torch.float32))
        t1, t2 = toks
        K = kps1.shape[0]
        if K == 0:
            return torch.empty(0, 2, dtype=torch.int64, device=t1.device)
        q = _sample(t1[None], kps1[None, :, :2].to(t1.device), gh, gw, pitch, img_h, img_w, query_patch, query_stride)[0]
        q = ops.l2_normalize(q.contiguous())
        S = ops.gemm_nt(q, t2, out_dtype=torch.float32)                    # [K, gh * pitch], exact fp32
        return ops.transfer_argmax(S.view(K, gh, pitch), (img_h, img_w), patch_size, stride)


def transfer_keypoints(module, img1, img2, kps1, img_size=640):
    """The reference's per-pair semantic transfer (src/evaluate_timm.py:509-547) on the HIP path: img1, img2 [3, img, img] fp32 in
    [0, 1] (already resized), kps1 [K, >= 2] (x, y, ...) -> kps_1_to_2 [K, 2] int64 (x, y) in view 2."""
    img_h, img_w = _img_hw(img_size)
    for im in (img1, img2):
        if tuple(im.shape[-2:]) != (img_h, img_w):
            raise GdHipError(f"image {tuple(im.shape[-2:])} is not img_size {(img_h, img_w)}")
    _, P, st = _backbone(module)
    g1, gh, gw, pitch = token_maps(module, img1)
    g2, _, _, _ = token_maps(module, img2)
    return transfer_keypoints_from_tokens(g1[0], g2[0], kps1, (img_h, img_w), P, st, pitch=pitch)


def semantic_transfer_pck(module, pairs, img_size=640, alphas=(0.10, 0.05, 0.15)):
    """PCK-Transfer of src/evaluate_timm.py:461-566 over already-loaded pairs (img1, img2, kps1, kps2): kps [K, 3] (x, y, visibility),
    images as `transfer_keypoints` takes them.  The visible keypoints (v1 * v2 > 0) of all pairs are pooled, as the reference pools
    a category -> {"PCK0.10": ..., ...} in `alphas` order, plus "n" (pooled keypoints)."""
    preds, gts = [], []
    for img1, img2, kps1, kps2 in pairs:
        xy = transfer_keypoints(module, img1, img2, kps1, img_size).cpu()
        k2 = kps2.cpu()
        vis = kps1[:, 2].cpu() * k2[:, 2] > 0
        gts.append(k2[vis][:, [1, 0]])
        preds.append(xy[vis][:, [1, 0]])
    if not gts or sum(len(g) for g in gts) == 0:
        raise GdHipError("semantic_transfer_pck: no visible keypoints")
    res = pck(torch.cat(preds), torch.cat(gts), img_size if isinstance(img_size, int) else max(_img_hw(img_size)), alphas)
    out = {f"PCK{a:.2f}": float(v) for a, v in zip(alphas, res.tolist())}
    out["n"] = int(sum(len(g) for g in gts))
    return out


# ----------------------------------------------------------------------------------------------------------------- TAP-Vid tracking
# src/evaluate_timm.py:234-348 (tracking_single / tracking) on utils/tracking_model.py (Tracker, ModelInference) and
# utils/tracking_metrics.py.  Defaults: patch 16, stride patch // 2, radius 35, anchor cosine 0.7, visibility cosine 0.6.
def track_geometry(img_h, img_w, patch, stride, pitch=None):
    """(img_h, img_w, patch, stride, gh, gw, pitch) of a tracking video: the grid is 1 + (img - patch) // stride per axis."""
    gh, gw = token_grid(img_h, img_w, patch, stride)
    return (int(img_h), int(img_w), int(patch), int(stride), gh, gw, gw if pitch is None else int(pitch))


def grid_xy(geom):
    """Pixel position of every cell of the gh x gw grid, raster order -> fp64 [gh * gw, 2] (x, y) = (col * s + p // 2, row * s + p // 2)
    (TrackerHead.soft_argmax's gen_grid, tracking_model.py:151-156)."""
    _, _, p, s, gh, gw, _ = geom
    yy, xx = torch.meshgrid(torch.arange(gh, dtype=torch.float64), torch.arange(gw, dtype=torch.float64), indexing="ij")
    return torch.stack([xx * s + p // 2, yy * s + p // 2], -1).reshape(-1, 2)


def disc_cells(geom, radius, cell):
    """Raster indices of the cells whose centre lies within `radius` pixels of cell `cell`'s (integer dx^2 + dy^2 <= r^2)."""
    _, _, p, s, gh, gw, _ = geom
    cy, cx = divmod(int(cell), gw)
    out = []
    for y in range(gh):
        for x in range(gw):
            if ((x - cx) * s) ** 2 + ((y - cy) * s) ** 2 <= radius * radius:
                out.append(y * gw + x)
    return out


def lower_median(x, dim=0):
    """torch.median's value along `dim`: for an even count the lower of the two middle values."""
    return torch.sort(x, dim=dim).values.select(dim, (x.shape[dim] - 1) // 2)


def video_token_maps(module, frames, stride=None, chunk=8):
    """Dense per-frame token maps for tracking (src/evaluate_timm.py:259-282): the patch stride is overridden to `stride` (default
    patch // 2) for this call only, frames [T, 3, H, W] CUDA fp32 in [0, 1] run through `token_maps` in chunks of `chunk`.
    -> (fmap [T, gh * pitch, D] fp32, gh, gw, pitch)."""
    m, P, st0 = _backbone(module)
    s = P // 2 if stride is None else int(stride)
    frames = _image(frames)
    old = m.patch_embed.proj.stride
    m.patch_embed.proj.stride = (s, s)
    try:
        maps, geo = [], None
        for i in range(0, frames.shape[0], max(1, int(chunk))):
            fm, gh, gw, pitch = token_maps(module, frames[i:i + chunk])
            maps.append(fm.float().contiguous())
            geo = (gh, gw, pitch)
        return (torch.cat(maps) if len(maps) > 1 else maps[0]), geo[0], geo[1], geo[2]
    finally:
        m.patch_embed.proj.stride = old


def _sample_frames(fmap, geom, pts, frames):
    """Bilinear samples (grid_sample align_corners=True, border; the (patch, stride) mapping of normalize_points_for_sampling) of
    fmap at pts [R, 2] in frame frames[R] -> [R, D] fp32, rows in input order."""
    img_h, img_w, p, s, gh, gw, pitch = geom
    R = pts.shape[0]
    out = torch.empty(R, fmap.shape[-1], dtype=torch.float32, device=fmap.device)
    fr = frames.cpu()
    for t in torch.unique(fr).tolist():
        idx = (fr == t).nonzero().reshape(-1).to(fmap.device)
        out[idx] = _sample(fmap[t:t + 1], pts.index_select(0, idx)[None], gh, gw, pitch, img_h, img_w, p, s)[0]
    return out


def track_queries(fmap, geom, query_points, *, radius=35, anchor_cos=0.7, cos_th=0.6, precision="f16", want_occlusion=True,
                  features=None):
    """ModelInference.infer (utils/tracking_model.py:578-594, batch_size=None) on gd_track_points.
    fmap [T, gh * pitch, D] (video_token_maps), geom = track_geometry(...), query_points [N, 3] (x, y, t) in pixels of the frames.
    -> (tracks [N, T, 2] fp32 (x, y), occluded [N, T] bool).  `features`: a prepared ops.TrackFeatures of fmap (reused across calls).
    Raises GdHipError for a query whose anchor set is empty (where the reference's torch.median of an empty tensor fails)."""
    with torch.no_grad():
        T = fmap.shape[0]
        dev = fmap.device
        tf = features if features is not None else ops.TrackFeatures(fmap, precision)
        q = query_points.to(dev, torch.float32).reshape(-1, 3)
        N = q.shape[0]
        tq = q[:, 2].round().long()
        if N == 0:
            return torch.empty(0, T, 2, device=dev), torch.zeros(0, T, dtype=torch.bool, device=dev)
        if int(tq.min()) < 0 or int(tq.max()) >= T:
            raise GdHipError(f"track_queries: query frames must lie in [0, {T})")
        # step 4: the query embedding against every frame
        emb = _sample_frames(fmap, geom, q[:, :2].contiguous(), tq)                               # [N, D]
        tiles = []
        for t in range(T):
            for r0 in range(0, N, 128):
                tiles.append([t, r0, min(128, N - r0), t * N + r0])
        traj = ops.track_points(emb, tf, geometry=geom, radius=radius, precision=precision, tiles=tiles).view(T, N, 2)
        tracks = traj.transpose(0, 1).contiguous()                                               # [N, T, 2]
        if not want_occlusion:
            return tracks, torch.zeros(N, T, dtype=torch.bool, device=dev)
        # step 5: samples along the trajectory, cosine against the trajectory's own point in the query frame
        tframes = torch.arange(T, device=dev).repeat(N)
        samp = _sample_frames(fmap, geom, tracks.reshape(-1, 2), tframes).view(N, T, -1)         # [N, T, D]
        ref = samp[torch.arange(N, device=dev), tq.to(dev)]                                       # [N, D]
        cos = torch.nn.functional.cosine_similarity(ref[:, None], samp, dim=-1, eps=1e-8)          # [N, T]
        anchors = (cos >= anchor_cos).cpu()                                                       # the one host sync of the video
        cnt = anchors.sum(1)
        if int(cnt.min()) == 0:
            bad = int((cnt == 0).nonzero()[0, 0])
            raise GdHipError(f"track_queries: query {bad} ({query_points[bad].tolist()}) has no anchor frame (cos >= {anchor_cos})")
        # step 6: every trajectory sample against every anchor frame, rows grouped by anchor frame into full tiles
        nn_, aa = anchors.nonzero(as_tuple=True)                                                  # (query, anchor) pairs
        rows = (nn_[:, None] * T + torch.arange(T)[None]).reshape(-1)                             # sample rows n*T + t
        frames = aa[:, None].expand(-1, T).reshape(-1)
        green = ops.track_points(samp.reshape(N * T, -1).index_select(0, rows.to(dev)), tf, frames=frames, geometry=geom,
                                 radius=radius, precision=precision).view(-1, T, 2)              # [pairs, T, 2]
        # step 7: occlusion from the anchors' cycle distances
        occ = torch.empty(N, T, dtype=torch.bool, device=dev)
        start = 0
        for n in range(N):
            k = int(cnt[n])
            a_idx = aa[start:start + k].to(dev)
            d = torch.linalg.norm(green[start:start + k] - tracks[n, a_idx][:, None], dim=-1)     # [A, T]
            med = lower_median(d, 0)                                                               # [T]
            th = med[a_idx].max()
            occ[n] = (med > th) | (cos[n] < cos_th)
            start += k
        return tracks, occ


# ---- TAP-Vid metrics (utils/tracking_metrics.py:7-221), numpy ------------------------------------------------------------------
def compute_tapvid_metrics(query_points, gt_occluded, gt_tracks, pred_occluded, pred_tracks, query_mode, get_trackwise_metrics=False):
    """TAP-Vid metrics (occlusion accuracy, pts_within_{1,2,4,8,16}, jaccard_{...}, the two averages) on [b, n, ...] arrays in
    256-scaled raster coordinates; query_points [b, n, 3] (t, y, x).  query_mode 'first' (frames after the query) or 'strided'
    (every frame but the query's).  -> dict of arrays [b] (or [b, n] with get_trackwise_metrics)."""
    import numpy as np
    axes = (2,) if get_trackwise_metrics else (1, 2)
    T = gt_tracks.shape[2]
    eye = np.eye(T, dtype=np.int32)
    if query_mode == "first":
        evalf = np.cumsum(eye, axis=1) - eye
    elif query_mode == "strided":
        evalf = 1 - eye
    else:
        raise ValueError("Unknown query mode " + query_mode)
    ev = evalf[np.round(query_points[..., 0]).astype(np.int32)] > 0
    out = {"occlusion_accuracy": np.sum(np.equal(pred_occluded, gt_occluded) & ev, axis=axes) / np.sum(ev, axis=axes)}
    vis, pvis = np.logical_not(gt_occluded), np.logical_not(pred_occluded)
    fracs, jacs = [], []
    for th in (1, 2, 4, 8, 16):
        within = np.sum(np.square(pred_tracks - gt_tracks), axis=-1) < np.square(th)
        correct = np.logical_and(within, vis)
        n_vis = np.sum(vis & ev, axis=axes)
        frac = np.sum(correct & ev, axis=axes) / n_vis
        tp = np.sum(correct & pvis & ev, axis=axes)
        fp = np.sum((((~vis) & pvis) | ((~within) & pvis)) & ev, axis=axes)
        jac = tp / (n_vis + fp)
        out[f"pts_within_{th}"], out[f"jaccard_{th}"] = frac, jac
        fracs.append(frac)
        jacs.append(jac)
    out["average_jaccard"] = np.mean(np.stack(jacs, axis=1), axis=1)
    out["average_pts_within_thresh"] = np.mean(np.stack(fracs, axis=1), axis=1)
    return out


def compute_tapvid_metrics_for_video(trajectories_dict, occlusions_dict, benchmark_data, video_idx, pred_video_sizes=None):
    """utils/tracking_metrics.py:150-221: the per-query-frame predictions {frame: [n, T, 2]} / {frame: [n, T]} of one video against
    its benchmark entry, scaled to 256 x 256 ('strided' queries) -> {metric: float}.  The reference's query-point rescale writes
    column 1 from column 2 and then column 2 from the NEW column 1 (:203-204); only column 0 (the frame) is read afterwards, so
    the quirk is kept and has no effect."""
    import numpy as np
    cfg = next(v for v in benchmark_data["videos"] if v["video_idx"] == video_idx)
    rh = cfg["h"] if pred_video_sizes is None else pred_video_sizes[1]
    rw = cfg["w"] if pred_video_sizes is None else pred_video_sizes[0]
    qp, gto, gtt, po, pt = [], [], [], [], []
    for f in cfg["query_points"]:
        q = np.array(cfg["query_points"][f])
        qp.append(np.concatenate([np.array([f] * q.shape[0])[:, None], q], axis=1))
        gtt.append(cfg["target_points"][f])
        gto.append(cfg["occluded"][f])
        pt.append(trajectories_dict[f])
        po.append(occlusions_dict[f])
    qp = np.concatenate(qp, axis=0, dtype=np.float32)
    gtt = np.concatenate(gtt, axis=0, dtype=np.float32)
    gto = np.concatenate(gto, axis=0, dtype=object)
    pt = np.concatenate(pt, axis=0, dtype=np.float32)
    po = np.concatenate(po, axis=0, dtype=object)
    qp[..., 1] = qp[..., 2] * 256 / cfg["h"]
    qp[..., 2] = qp[..., 1] * 256 / cfg["w"]
    gtt[..., 0] *= 256 / cfg["w"]
    gtt[..., 1] *= 256 / cfg["h"]
    pt[..., 0] *= 256 / rw
    pt[..., 1] *= 256 / rh
    m = compute_tapvid_metrics(qp[None], gto[None], gtt[None], po[None], pt[None], query_mode="strided")
    return {k: v.item() for k, v in m.items()}


def tapvid_video_metrics(module, frames, video_config, *, patch=None, stride=None, radius=35, anchor_cos=0.7, cos_th=0.6,
                         precision="f16", chunk=8):
    """tracking_single (src/evaluate_timm.py:234-335) on already-decoded frames [T, 3, H, W] (CUDA fp32 in [0, 1], resized by the
    caller to H, W floored to multiples of the patch) and the video's benchmark dict (the strided-pkl entry: video_idx, h, w,
    query_points, target_points, occluded).  -> {metric: float, ..., "video_idx": int}."""
    _, P, _ = _backbone(module)
    s = P // 2 if stride is None else int(stride)
    H, W = frames.shape[-2:]
    fmap, gh, gw, pitch = video_token_maps(module, frames, stride=s, chunk=chunk)
    geom = (int(H), int(W), P if patch is None else int(patch), s, gh, gw, pitch)
    tf = ops.TrackFeatures(fmap, precision)
    fx, fy = W / video_config["w"], H / video_config["h"]
    trajs, occs = {}, {}
    for f in sorted(video_config["query_points"].keys()):
        q = torch.tensor([[fx * p[0], fy * p[1], f] for p in video_config["query_points"][f]], dtype=torch.float32)
        tr, oc = track_queries(fmap, geom, q, radius=radius, anchor_cos=anchor_cos, cos_th=cos_th, precision=precision,
                               features=tf)
        trajs[f], occs[f] = tr.cpu().numpy(), oc.cpu().numpy()
    m = compute_tapvid_metrics_for_video(trajs, occs, {"videos": [video_config]}, video_config["video_idx"], pred_video_sizes=[W, H])
    m["video_idx"] = int(video_config["video_idx"])
    return m


def tracking(module, videos, **kw):
    """tracking (src/evaluate_timm.py:338-348) over already-decoded videos [(frames, video_config), ...] -> (table: one metric dict per
    video, mean: every metric's mean over the videos).  The reference's callback logs metrics_df.iloc[:, 1:].mean(), which drops the
    first column (occlusion_accuracy); `mean` keeps every column."""
    table = [tapvid_video_metrics(module, fr, cfg, **kw) for fr, cfg in videos]
    keys = [k for k in table[0] if k != "video_idx"] if table else []
    mean = {k: sum(r[k] for r in table) / len(table) for k in keys}
    return table, mean
