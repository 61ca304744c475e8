"""The frozen teacher, run ONCE per image pair, feeding `teacher_cache.TeacherTargetCache` (north_star: "the frozen teacher
(mast3r/model.py, vggt/models) runs once per pair on-device via cached PyTorch-ROCm inference").

The teacher networks are the USER'S modules (the reference vendors them; they are not part of this repository and stay plain
PyTorch-ROCm inference).  What lives here is the glue around them:

* `QKCapture` — forward hooks that pick the post-norm, post-RoPE q and k of selected attention modules off a running teacher
  (duck-typed on the attribute names of `vggt/layers/attention.py:24-50`: `qkv`, `q_norm`, `k_norm`, `rope`, `num_heads`), so the
  distillation target maps can be built by `gd_cross_view_attn` WITHOUT the [2B, H, n, n] per-head softmax maps the reference's
  `return_attn` branch materialises (`vggt/layers/attention.py:73-84`: 480 MB per pair and block at n = 1369);
* `VGGTTeacherRunner` — `extract_vggt_features` + `sample_keypoints` (src/finetune_timm_vggt.py:357-449) as one call that returns the
  pair's targets in the cache layout; the reference aggregator's hard-wired `return_attn=True` is neutralised for the duration of the
  call (the selected blocks return a 1-element placeholder instead of the maps); with `fused_heads` the three dense-prediction heads run on
  the HIP kernels (teacher_heads.FusedDPTHead) instead of the user's modules, with `fused_tracker` the tracker's tail runs on
  teacher_tracker.FusedTracker, with `fused_patch_embed` the aggregator's DINOv2 patch embedder runs on teacher_blocks.FusedDinoEmbed, and with
  `fused_camera_head` the camera head runs on teacher_heads.FusedCameraHead;
* `MASt3RTeacherRunner` — `extract_mast3r_features` + `filter_and_match_keypoints` + the depth branch
  (src/finetune_timm_mast3r.py:345-469, 617-633) around the user's `dust3r.inference.inference`.
"""
import contextlib

import torch

from . import teacher_glue as tg
from ._lib import GdHipError


class QKCapture:
    """with QKCapture(attn_modules) as cap: teacher(...);  cap.qk -> [(q, k)] per module call, each [B, H, N, d] as they enter
    the attention product (after q_norm / k_norm and RoPE).  Works on any module shaped like vggt's `Attention`."""

    def __init__(self, attn_modules):
        self.mods = list(attn_modules)
        self.qk, self._h, self._pend = [], [], {}

    def __enter__(self):
        self._active = None
        ropes = {}
        for i, m in enumerate(self.mods):
            # which selected module is executing: the RoPE module is typically ONE object shared by every block of the teacher
            # (vggt/models/aggregator.py:77-96 hands `self.rope` to all frame and global blocks), so its hook must know whose
            # call it is seeing
            self._h.append(m.register_forward_pre_hook(lambda mod, a, i=i: setattr(self, "_active", i)))
            self._h.append(m.register_forward_hook(lambda mod, a, out: setattr(self, "_active", None)))
            rope = getattr(m, "rope", None)
            if rope is not None and isinstance(rope, torch.nn.Module):
                ropes[id(rope)] = rope        # forward() calls self.rope(q, pos) then self.rope(k, pos): outputs arrive in that order
            else:
                for nm in ("q_norm", "k_norm"):
                    if not isinstance(getattr(m, nm, None), torch.nn.Module):
                        raise GdHipError(f"QKCapture: module {type(m).__name__} has neither a rope module nor {nm}")
                self._h.append(m.q_norm.register_forward_hook(lambda mod, a, out: self._push(out)))
                self._h.append(m.k_norm.register_forward_hook(lambda mod, a, out: self._push(out)))
        for rope in ropes.values():
            self._h.append(rope.register_forward_hook(lambda mod, a, out: self._push(out)))
        return self

    def _push(self, out):
        i = self._active
        if i is None:
            return
        lst = self._pend.setdefault(i, [])
        lst.append(out.detach())
        if len(lst) == 2:
            self.qk.append((i, lst[0], lst[1]))
            self._pend[i] = []

    def __exit__(self, *exc):
        for h in self._h:
            h.remove()
        self._h = []
        return False

    def pairs(self):
        """[(q, k)] ordered by module index (one call per module assumed)."""
        return [(q, k) for _, q, k in sorted(self.qk, key=lambda t: t[0])]


@contextlib.contextmanager
def _no_attention_maps(attn_modules):
    """The reference's aggregator calls its global blocks with return_attn=True unconditionally (vggt/models/aggregator.py:257,
    314) and each then forms two [B, H, n, n] softmax maps.  For the duration of the block, the selected attention modules answer
    `return_attn=True` with (output, 1-element placeholder): the aggregator's `torch.stack(attn_list).mean(0)` stays valid, the
    maps are never built."""
    saved = []
    for m in attn_modules:
        orig = m.forward

        def fwd(x, pos=None, return_attn=False, temperature=1.0, _orig=orig):
            out = _orig(x, pos=pos)
            return (out, out.new_zeros(1)) if return_attn else out
        saved.append((m, orig))
        m.forward = fwd
    try:
        yield
    finally:
        for m, orig in saved:
            del m.forward            # drop the instance attribute: the class's forward is visible again


@contextlib.contextmanager
def _shadowed(*triples):
    """For the duration of the block, each (object, name, value) is an instance attribute that shadows the class's method of that name (a
    module's `forward`, the matcher's `_decoder`): the user's own code drives the fused path.  Deleted again, last first, however the block ends."""
    done = []
    try:
        for obj, name, value in triples:
            setattr(obj, name, value)
            done.append((obj, name))
        yield
    finally:
        for obj, name in reversed(done):
            delattr(obj, name)                      # the class's own attribute is visible again


class VGGTTeacherRunner:
    """vggt: a model shaped like vggt.models.vggt.VGGT (aggregator with `global_blocks`, `attn_indices`, `aa_block_size`,
    `temperature`; camera_head, depth_head, point_head, track_head).  `pose_decoder(pose_enc, image_hw) -> (extrinsic, intrinsic)`
    = vggt.utils.pose_enc.pose_encoding_to_extri_intri of the user's vggt package (imported lazily when not given)."""

    def __init__(self, vggt, dtype=torch.bfloat16, prefix=5, pose_decoder=None, fused_blocks=False, fused_heads=False, heads_dtype=torch.float32,
                 fused_updateformer=False, *, fused_patch_embed=False, fused_camera_head=False, camera_dtype=torch.float32, tracker_linear="gemm_nt",
                 fused_tracker=False):
        if fused_updateformer and not fused_tracker:
            raise GdHipError("VGGTTeacherRunner: fused_updateformer=True needs fused_tracker=True (the fused update transformer runs inside FusedTracker's loop)")
        if tracker_linear != "gemm_nt" and not fused_tracker:
            raise GdHipError(f"VGGTTeacherRunner: tracker_linear={tracker_linear!r} needs fused_tracker=True (it chooses the linear kernel of FusedTracker and its "
                             f"FusedUpdateFormer)")
        self.m, self.dtype, self.prefix, self.pose_decoder = vggt, dtype, prefix, pose_decoder
        agg = vggt.aggregator
        per = getattr(agg, "aa_block_size", 1)
        # aggregator.forward appends the map of the LAST global block of every selected aa iteration (aggregator.py:255-260)
        self.sel = [agg.global_blocks[i * per + per - 1].attn for i in agg.attn_indices]
        # fused_blocks: the 2 x depth attention blocks run on the HIP kernels (teacher_blocks.FusedAggregatorBlocks) instead of the user's modules
        self.fused = None
        if fused_blocks:
            from .teacher_blocks import FusedAggregatorBlocks
            self.fused = FusedAggregatorBlocks(agg, dtype=dtype)
        # fused_heads: the three dense-prediction heads run on the HIP kernels (teacher_heads.FusedDPTHead, operand type `heads_dtype`: torch.float32 is
        # the faithful mode, the reference runs its heads in fp32).  Independent of fused_blocks; a head the class refuses raises here, not in targets().
        self.heads = None
        if fused_heads:
            from .teacher_heads import FusedDPTHead
            self.heads = {n: FusedDPTHead(h, dtype=heads_dtype, name=n) for n, h in (("depth_head", vggt.depth_head), ("point_head", vggt.point_head),
                                                                                      ("track_head.feature_extractor", vggt.track_head.feature_extractor))}
        # fused_tracker: the tracker's correlation pyramid, window sampling, position embedding, glue and small MLPs run on the HIP kernels
        # (teacher_tracker.FusedTracker, fp32; the update transformer stays the user's module unless fused_updateformer, off by default, hands it to
        # teacher_tracker.FusedUpdateFormer; pass both by keyword, fused_tracker stays the last one — keyword only since fused_patch_embed, which is keyword only,
        # stands in front of it).  tracker_linear (keyword only, "gemm_nt" by default): "tokens" runs the linear layers of the fused tracker and of its
        # fused update transformer on gd_tokens_linear, the small-tile fp32 kernel for their few hundred rows.  Independent of fused_blocks and
        # fused_heads; a tracker the class refuses raises here, not in targets().
        self.tracker = None
        if fused_tracker:
            from .teacher_tracker import FusedTracker
            self.tracker = FusedTracker(vggt.track_head.tracker, name="track_head.tracker", fused_updateformer=fused_updateformer, linear=tracker_linear)

        # fused_patch_embed (keyword only): the aggregator's DINOv2 patch embedder runs on the HIP kernels (teacher_blocks.FusedDinoEmbed, operand type
        # `dtype`).  Independent of the other switches; an embedder, or an aggregator around it, that the class refuses raises here, not in targets().
        self.embed = None
        if fused_patch_embed:
            from .teacher_blocks import FusedDinoEmbed
            if not hasattr(agg, "patch_embed"):
                raise GdHipError("VGGTTeacherRunner: fused_patch_embed=True: the aggregator has no `patch_embed`")
            self.embed = FusedDinoEmbed(agg.patch_embed, dtype=dtype, name="aggregator.patch_embed")
            self.embed.check_aggregator(agg)
        # fused_camera_head (keyword only): the camera head runs on the few-row HIP kernels (teacher_heads.FusedCameraHead, weight type `camera_dtype`:
        # torch.float32 is the faithful mode, the reference runs this head in fp32).  Independent of the other switches; a head the class refuses raises
        # here, not in targets().
        self.camera = None
        if fused_camera_head:
            from .teacher_heads import FusedCameraHead
            self.camera = FusedCameraHead(vggt.camera_head, dtype=camera_dtype, name="camera_head")

    def _block_inputs(self, rgb_vggt):
        """What the aggregator hands its first frame block, produced by the aggregator itself: its forward runs as it stands (normalisation, the
        user's patch embedder, camera / register tokens, position grid) and is left where the blocks begin.  -> tokens [B*S, P, C], pos [B*S, P, 2]."""
        class _AtBlocks(Exception):
            pass
        got = {}

        def stop(mod, args, kwargs):
            got["tokens"], got["pos"] = args[0], kwargs.get("pos", args[1] if len(args) > 1 else None)
            raise _AtBlocks
        h = self.m.aggregator.frame_blocks[0].register_forward_pre_hook(stop, with_kwargs=True)
        try:
            self.m.aggregator(rgb_vggt)
        except _AtBlocks:
            pass
        finally:
            h.remove()
        if got.get("pos") is None:
            raise GdHipError("VGGTTeacherRunner: the aggregator gave its first frame block no positions (rope off?): fused_blocks cannot serve it")
        return got["tokens"], got["pos"]

    @torch.no_grad()
    def aggregate(self, rgb_vggt):
        """rgb_vggt [B, S, 3, H, W] -> (tokens_list, ps_idx, qk_or_maps): the aggregator's token outputs and patch start index, and what the
        cross-view target is built from — the selected global blocks' [(q, k)] off the user's modules (hooks), or, with fused_blocks, the
        finished maps [2B, n, n]."""
        agg = self.m.aggregator
        if self.fused is not None:
            B, S = rgb_vggt.shape[:2]
            if self.embed is not None:
                tokens, pos = self.embed.aggregator_tokens(rgb_vggt, agg)         # neither the aggregator's forward nor the module's is called
            else:
                with torch.autocast("cuda", dtype=self.dtype, enabled=rgb_vggt.is_cuda and self.dtype != torch.float32):
                    tokens, pos = self._block_inputs(rgb_vggt)
            tokens_list, maps = self.fused.forward(tokens, pos, B, S)
            return tokens_list, agg.patch_start_idx, maps
        # with fused_patch_embed, for this call only, the user's aggregator drives the fused embedder
        shadow = [(agg.patch_embed, "forward", self.embed.forward)] if self.embed is not None else []
        with _shadowed(*shadow), QKCapture(self.sel) as cap, _no_attention_maps(self.sel):
            with torch.autocast("cuda", dtype=self.dtype, enabled=rgb_vggt.is_cuda):
                tokens_list, ps_idx, _ = agg(rgb_vggt)
        qk = [(q.to(self.dtype) if q.dtype not in (torch.float32, torch.bfloat16) else q,
               k.to(self.dtype) if k.dtype not in (torch.float32, torch.bfloat16) else k) for q, k in cap.pairs()]
        return tokens_list, ps_idx, qk

    @torch.no_grad()
    def cameras(self, tokens_list, image_hw):
        """-> (extrinsic [B, S, 3, 4], intrinsic [B, S, 3, 3]) of the last refinement iteration: the user's camera head then `pose_decoder` (or the lazily
        imported one); with fused_camera_head, FusedCameraHead.poses — or, when a `pose_decoder` was given, FusedCameraHead.forward through that decoder."""
        dec = self.pose_decoder
        if self.camera is not None and dec is None:
            _, extrinsic, intrinsic = self.camera.poses(tokens_list, image_hw)
            return extrinsic, intrinsic
        pose_enc = (self.camera if self.camera is not None else self.m.camera_head)(tokens_list)[-1]
        if dec is None:
            from vggt.utils.pose_enc import pose_encoding_to_extri_intri as dec       # the user's teacher package
        return dec(pose_enc, image_hw)

    @torch.no_grad()
    def targets(self, rgb_vggt, num_keypoints=300, min_distance=5, generator=None):
        """rgb_vggt [1, 2, 3, H, W] in [0, 1] -> the pair's target dict (teacher_glue.extract_vggt_targets), or None."""
        m, agg = self.m, self.m.aggregator
        tokens_list, ps_idx, qk = self.aggregate(rgb_vggt)
        extrinsic, intrinsic = self.cameras(tokens_list, rgb_vggt.shape[-2:])
        heads = self.heads
        depth_map, _ = (heads["depth_head"] if heads else m.depth_head)(tokens_list, rgb_vggt, ps_idx)
        _, point_conf = (heads["point_head"] if heads else m.point_head)(tokens_list, rgb_vggt, ps_idx)

        def track(kp1):
            if self.tracker is not None:
                # the feature extractor's map goes straight to the fused tracker: channel-last from the fused head, NCHW from the user's
                iters = int(getattr(m.track_head, "iters", 4))
                if heads:
                    fm, pitch = heads["track_head.feature_extractor"](tokens_list, rgb_vggt, ps_idx, channel_last=True)
                    trk, _, _ = self.tracker(kp1[None], iters=iters, fmaps_cl=fm, pitch=pitch)
                else:
                    trk, _, _ = self.tracker(kp1[None], m.track_head.feature_extractor(tokens_list, rgb_vggt, ps_idx), iters=iters)
                return trk[-1][0][1]
            # with fused heads, for this call only, the user's track_head drives the fused feature extractor
            shadow = [(m.track_head.feature_extractor, "forward", heads["track_head.feature_extractor"].forward)] if heads else []
            with _shadowed(*shadow):
                trk, _, _ = m.track_head(tokens_list, rgb_vggt, ps_idx, query_points=kp1[None])
            return trk[-1][0][1]
        fused = self.fused is not None
        scale = float(self.sel[0].scale) if hasattr(self.sel[0], "scale") else (64 if fused else qk[0][0].shape[-1]) ** -0.5
        return tg.extract_vggt_targets(None if fused else qk, depth_map[0], point_conf[0], extrinsic[0], intrinsic[0], track, scale=scale,
                                       temperature=float(getattr(agg, "temperature", 1.0)), prefix=self.prefix,
                                       num_keypoints=num_keypoints, min_distance=min_distance, generator=generator,
                                       maps=qk if fused else None)


class MASt3RTeacherRunner:
    """matcher: the user's AsymmetricMASt3R (the reference's fork returns `tgt_attn_map`, dust3r/dust3r/model.py:346-366);
    `inference` / `make_pairs`: dust3r.inference.inference and dust3r.image_pairs.make_pairs of the user's package (lazy import).

    fused_blocks: the encoder and decoder blocks run on the HIP kernels (teacher_blocks.FusedCroCoBlocks, operand type `dtype`: torch.float32
    is the faithful mode, the reference runs this teacher in fp32; torch.bfloat16 is narrower and faster).  For the duration of `targets()`
    only, instance attributes shadow `matcher._decoder` (by FusedCroCoBlocks.decode) and every `enc_blocks[i].forward` (the first runs the whole
    stack, the others return their input), so the user's own `forward` — patch embedding, `enc_norm`, heads — drives the fused path.  The
    shadowed `_decoder` returns one-head head-mean score maps [B, 1, Nq, Nk], which `forward`'s and this class's `.mean(dim=1)` leave unchanged.

    fused_heads: `downstream_head1` and `downstream_head2` run on the HIP kernels (teacher_heads.FusedMASt3RHead, operand type `heads_dtype`:
    torch.float32 is the faithful mode, the reference runs its heads in fp32 with autocast off).  Independent of `fused_blocks`; a head the class
    does not serve raises here, naming the attribute.  For the duration of `targets()` only, an instance attribute shadows each module's `forward`,
    so the `head1` / `head2` closures the matcher built around those modules (portrait / landscape handling) keep driving the fused path."""

    def __init__(self, matcher, inference=None, make_pairs=None, min_conf_thr=10, subsample=16, keep_logits=False, fused_blocks=False,
                 dtype=torch.float32, fused_heads=False, heads_dtype=torch.float32):
        self.matcher, self.inference, self.make_pairs = matcher, inference, make_pairs
        self.min_conf_thr, self.subsample, self.keep_logits = min_conf_thr, subsample, keep_logits
        self.fused = None
        if fused_blocks:
            from .teacher_blocks import FusedCroCoBlocks
            self.fused = FusedCroCoBlocks(matcher, dtype=dtype)
        self.heads = None
        if fused_heads:
            from . import teacher_heads
            self.heads = {n: teacher_heads.FusedMASt3RHead(getattr(matcher, n), dtype=heads_dtype, name=n) for n in ("downstream_head1", "downstream_head2")}

    @torch.no_grad()
    def targets(self, rgb_mast3r_1, rgb_mast3r_2, temperature=1.0, intrinsic=None, depth_1=None, depth_2=None, device="cuda"):
        inf, mk = self.inference, self.make_pairs
        if inf is None:
            from dust3r.inference import inference as inf
        if mk is None:
            from dust3r.image_pairs import make_pairs as mk
        self.matcher.temperature = temperature          # src/finetune_timm_mast3r.py:215, 224: the annealed target temperature
        # the decoder's raw cross-attention score maps (dust3r/dust3r/model.py:337, `_decoder` -> dec_feats, tgt_camap, src_camap) are
        # picked up on the way: their head mean / reciprocity average is the temperature-independent part of `tgt_attn_map`, which
        # lets TeacherTargetCache(keep_logits=True) follow the annealed temperature without another teacher forward
        fused = self.fused
        seen, dec = [], fused.decode if fused is not None else getattr(self.matcher, "_decoder", None)
        shadow = []                                     # (object, name, value): see _shadowed
        if self.keep_logits and dec is not None:
            def wrapped(*a, **k):
                r = dec(*a, **k)
                if isinstance(r, tuple) and len(r) == 3:
                    seen.append((r[1], r[2]))
                return r
            shadow.append((self.matcher, "_decoder", wrapped))
        elif fused is not None:
            shadow.append((self.matcher, "_decoder", dec))
        if fused is not None:
            shadow += [(blk, "forward", fused.encode if i == 0 else (lambda x, pos=None: x)) for i, blk in enumerate(self.matcher.enc_blocks)]
        shadow += [(getattr(self.matcher, n), "forward", head.forward) for n, head in (self.heads or {}).items()]
        with _shadowed(*shadow):
            out = inf(mk([rgb_mast3r_1, rgb_mast3r_2], scene_graph="complete", prefilter=None, symmetrize=True), self.matcher, device,
                      verbose=False)
        p1, p2 = out["pred1"], out["pred2"]
        dev = torch.device(device)
        recip = tg.mast3r_recip_logits([t.to(dev) for t in seen[-1][0]], [t.to(dev) for t in seen[-1][1]]) if seen else None
        return tg.extract_mast3r_targets(
            p1["desc"][1].to(dev), p2["desc"][1].to(dev), p1["conf"][1].to(dev), p1["conf"][0].to(dev),
            p1["pts3d"][1].to(dev), p2["pts3d_in_other_view"][1].to(dev), p1["pts3d"][0].to(dev),
            p2["tgt_attn_map"][1].to(dev), p2["tgt_attn_map"][0].to(dev), intrinsic=intrinsic, depth_1=depth_1, depth_2=depth_2,
            subsample=self.subsample, min_conf_thr=self.min_conf_thr, cost_recip=recip)
