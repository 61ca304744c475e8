"""fp64 CPU restatement of the TAP-Vid tracker (utils/tracking_model.py Tracker + ModelInference.infer, batch_size=None):
steps 3-7 of the tracking evaluation on a feature volume feats [T, gh, gw, D].  A test helper, not a test module."""
import torch
import torch.nn.functional as F


def grid_xy(p, s, gh, gw):
    yy, xx = torch.meshgrid(torch.arange(gh, dtype=torch.float64), torch.arange(gw, dtype=torch.float64), indexing="ij")
    return torch.stack([xx * s + p // 2, yy * s + p // 2], -1).reshape(-1, 2)


def disc_mask(p, s, gh, gw, radius, cell):
    xy = grid_xy(p, s, gh, gw)
    d = xy - xy[int(cell)]
    return (d * d).sum(-1) <= radius * radius


def sample(feats, geom, pts, frames):
    """grid_sample(align_corners=True, border) at the (patch, stride) patch-centre mapping, pts [R, 2] (x, y) in pixels (fp32 values,
    mapped in fp64), frames [R] -> [R, D] fp64."""
    H, W, p, s, gh, gw = geom[:6]
    lh = ((H - p) // s) * s + p / 2
    lw = ((W - p) // s) * s + p / 2
    a = torch.tensor([2 / (lw - p / 2), 2 / (lh - p / 2)], dtype=torch.float64)
    b = torch.tensor([1 - lw * 2 / (lw - p / 2), 1 - lh * 2 / (lh - p / 2)], dtype=torch.float64)
    g = a * pts.double() + b
    out = torch.empty(pts.shape[0], feats.shape[-1], dtype=torch.float64)
    for t in torch.unique(frames).tolist():
        idx = (frames == t).nonzero().reshape(-1)
        v = F.grid_sample(feats[t].permute(2, 0, 1)[None].double(), g[idx][None, None], mode="bilinear", padding_mode="border",
                          align_corners=True)
        out[idx] = v[0, :, 0].T
    return out


def scores(e, Ft):
    """relu'd cosine map of embedding e [D] against frame Ft [gh, gw, D] -> (c [gh*gw], r [gh*gw]) fp64."""
    f = Ft.reshape(-1, Ft.shape[-1]).double()
    e = e.double()
    c = (f @ e) / torch.clamp(e.norm() * f.norm(dim=1), min=1e-8)
    return c, torch.relu(c)


def soft_argmax_at(r, geom, radius, cell):
    """sum_{disc(cell)} xy exp(r) / sum exp(r) -> [2] fp64."""
    _, _, p, s, gh, gw = geom[:6]
    m = disc_mask(p, s, gh, gw, radius, cell)
    w = torch.exp(r[m] - r.max())
    return (grid_xy(p, s, gh, gw)[m] * w[:, None]).sum(0) / w.sum()


def head(e, Ft, geom, radius):
    """The tracker head: (point [2], argmax cell) fp64."""
    _, r = scores(e, Ft)
    g = int(torch.argmax(r))
    return soft_argmax_at(r, geom, radius, g), g


def lower_median(x, dim=0):
    return torch.sort(x, dim=dim).values.select(dim, (x.shape[dim] - 1) // 2)


def infer(feats, geom, query_points, radius=35, anchor_cos=0.7, cos_th=0.6, traj_override=None):
    """-> dict(tracks [N, T, 2], occ [N, T] bool, cos [N, T], cells [N, T], samples [N, T, D], green {n: [A, T, 2]},
    anchors {n: [A]}).  traj_override: use these tracks [N, T, 2] for steps 5-7 (each stage on its own inputs)."""
    T = feats.shape[0]
    q = query_points.float()
    N = q.shape[0]
    tq = q[:, 2].round().long()
    emb = sample(feats, geom, q[:, :2], tq)
    tracks = torch.empty(N, T, 2, dtype=torch.float64)
    cells = torch.empty(N, T, dtype=torch.long)
    for n in range(N):
        for t in range(T):
            tracks[n, t], cells[n, t] = head(emb[n], feats[t], geom, radius)
    tr = tracks if traj_override is None else traj_override.double()
    samp = sample(feats, geom, tr.reshape(-1, 2), torch.arange(T).repeat(N)).view(N, T, -1)
    ref = samp[torch.arange(N), tq]
    cos = F.cosine_similarity(ref[:, None], samp, dim=-1, eps=1e-8)
    occ = torch.empty(N, T, dtype=torch.bool)
    green, anchors, meds = {}, {}, {}
    for n in range(N):
        A = (cos[n] >= anchor_cos).nonzero().reshape(-1)
        anchors[n] = A
        if A.numel() == 0:
            raise ValueError(f"query {n} has no anchor frame")
        gpts = torch.empty(A.numel(), T, 2, dtype=torch.float64)
        for i, a in enumerate(A.tolist()):
            for t in range(T):
                gpts[i, t] = head(samp[n, t], feats[a], geom, radius)[0]
        green[n] = gpts
        d = (gpts - tr[n, A][:, None]).norm(dim=-1)
        med = lower_median(d, 0)
        th = med[A].max()
        meds[n] = (med, th)
        occ[n] = (med > th) | (cos[n] < cos_th)
    return dict(tracks=tracks, occ=occ, cos=cos, cells=cells, samples=samp, green=green, anchors=anchors, meds=meds, emb=emb)
