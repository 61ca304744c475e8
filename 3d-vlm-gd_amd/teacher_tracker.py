"""The VGGT teacher's tracker tail (vggt/heads/track_modules/base_track_predictor.py:82-209 BaseTrackerPredictor.forward) on the HIP kernels of
csrc/vggt_track.hip and the existing GEMM / LayerNorm entry points, instead of the user's PyTorch module.

What the reference does in every iteration and this class does not:
  * it rebuilds the [1, 388, H, W] sin/cos position table on the host and copies it over (:149) to sample it at N points (:150) —
    here gd_track_pos_embed computes the N sampled rows once per call;
  * it writes the full correlation volume of every pyramid level (blocks.py:205-246) to read (2r+1)^2 values per point from it —
    here gd_corr_sample computes the (2r+2)^2 dot products a window needs and blends them; the volume never exists;
  * it permutes the feature map NCHW -> NHWC -> NCHW around `fmap_norm` (:94-95) — here every map is channel-last (`fmaps_cl=` takes the fused
    DPT head's map as it is, separator column included).

One iteration (`step`) is
    corr_sample -> gemm_nt(+bias, GELU) -> gemm_nt(+bias)            (the window samples, `corr_mlp`)
    track_assemble                                                    (flow embedding | flow / max_scale | corr | track_feats, + position + query token)
    updateformer                                                      (the USER'S module, called as it stands; FusedUpdateFormer with fused_updateformer=True)
    track_update                                                      (coords += delta[:2], frame 0 pinned; the prediction; delta[2:] as aligned rows)
    layernorm_fwd -> gemm_nt(+bias, GELU, +residual)                  (`ffeat_norm` — GroupNorm(1, C) on [M, C] rows is a row LayerNorm — and `ffeat_updater`)
and every row keeps the order (b, n, s) through the loop: nothing is permuted.

fp32 only.  The loop feeds its coordinates back through sin(~970 * flow) (utils.py:110-119: div_term reaches 62 * 1000 / 64) and amplifies rounding by
about an order of magnitude per iteration; with the reference's own modules, fp32 against fp64 already differs by up to a pixel after four iterations at
unit-scale `flow_head` weights.  A 16-bit operand mode would start that growth from 2^-9 instead of 2^-24 and is not offered.

The module stays the user's: this class reads its parameters (duck-typed on the attribute names, through teacher_read.Reader as teacher_blocks._ViTBlock does) and refuses, naming the
attribute, anything the kernels do not serve.  Off by default (teacher_runner.VGGTTeacherRunner(fused_tracker=True))."""
import torch

from . import ops
from ._lib import GdHipError
from .teacher_read import Reader, f32, to_device

C_LATENT, MAX_RADIUS, MAX_LEVELS = 128, 4, 8


def level_sizes(H, W, levels):
    """[(H_l, W_l)] of the pyramid (floor halving, blocks.py:168-176)."""
    out = [(int(H), int(W))]
    for _ in range(levels - 1):
        out.append((out[-1][0] // 2, out[-1][1] // 2))
    return out


def check_levels(H, W, levels, who="FusedTracker"):
    """A level whose map has a side of 1 (or 0) is refused: there the reference's 2 / max(size - 1, 1) normalisation sends every sample to cell 0,
    which the integer-window form does not reproduce."""
    for l, (h, w) in enumerate(level_sizes(H, W, levels)):
        if h < 2 or w < 2:
            raise GdHipError(f"{who}: level {l} of a {H} x {W} map is {h} x {w}: a pyramid level with a side below 2 is not served "
                             f"({levels} levels need sides of at least {2 ** levels})")


def _lin_bias(b, n, like):
    """The tracker's linear layers always hand their kernel a bias vector: zeros where the module has none."""
    return f32(b) if b is not None else torch.zeros(n, dtype=torch.float32, device=like.device)


def _bias(lin):
    return _lin_bias(lin.bias, lin.out_features, lin.weight)


LINEAR_KINDS = ("gemm_nt", "tokens")


def _linear_kind(linear, who):
    if linear not in LINEAR_KINDS:
        raise GdHipError(f"{who}: linear = {linear!r}: 'gemm_nt' (gd_gemm_nt, the default) or 'tokens' (gd_tokens_linear) are served")
    return linear


def _linear(kind, a, w, bias, act=0, residual=None, out=None, accumulate=False):
    """One fp32 linear layer of the tracker on gd_gemm_nt or, with kind "tokens", on gd_tokens_linear (the small-tile kernel for these row counts);
    act: 0 none, 1 exact GELU."""
    if kind == "tokens":
        return ops.tokens_linear(a, w, bias, out=out, residual=residual, gelu=act == 1, accumulate=accumulate)
    return ops.gemm_nt(a, w, out, bias=bias, act=act, residual=residual, accumulate=accumulate)


class FusedUpdateFormer:
    """FusedUpdateFormer(updateformer)(x [B, N, S, 3C + 4]) -> (delta [B, N, S, C + 2], None): the tracker's update transformer
    (vggt/heads/track_modules/blocks.py:19-144 EfficientUpdateFormer on modules.py:147-218 AttnBlock / CrossAttnBlock) on gd_layernorm_fwd, gd_gemm_nt
    and gd_attention_small_fwd, fp32 only.

    There is ONE token buffer [B, N + nv, S, D], rows in the order (b, n, s) the tracker loop keeps, the nv virtual tracks behind the points; no
    token tensor is permuted, concatenated or repeated per block, and the virtual rows are written once per call.
      * a time block takes every row: its sequences are S consecutive rows (G0 = B (N + nv), G1 = 1);
      * the space stage of frame (b, s) addresses tokens S rows apart (G0 = 1 per batch entry, G1 = S): `virtual2point` (q = virtual rows, k | v = ONE
        GEMM of norm_context(points) on in_proj_weight[D:]), `virtual` (self-attention on the virtual rows), `point2virtual`; the three write back into
        the same buffer, so the next time block reads it as it is.
    A sequence layout is (G0, G1, L, r0, r1, rl): token i of sequence (g0, g1) is row g0 * r0 + g1 * r1 + i * rl of the rows handed over.

    The teacher's block REPLACES x by norm1(x) (modules.py:174-183): the attention's residual is the normed x, not the block input; the same in the
    cross block.  The blocks whose point rows are the last ones written add them onto the saved input tokens (the GEMM's accumulate), so
    `tokens[:, :N] + init_tokens` costs no pass of its own; a last time block without a space stage runs on the point rows alone.

    linear="tokens" (off by default) sends every linear layer through gd_tokens_linear instead of gd_gemm_nt: the same products in exact fp32 on
    32 x 32 tiles whose four waves split K, for the few hundred rows this transformer sees.

    Read once, duck-typed on the attribute names; what the kernels do not serve is refused here, naming the attribute."""

    def __init__(self, former, name="updateformer", *, linear="gemm_nt"):
        self.name = name
        self.linear = _linear_kind(linear, f"FusedUpdateFormer: {name}")
        r = Reader("FusedUpdateFormer", name)
        fail, need = r.fail, r.need
        it, fh = need(former, "input_transform"), need(former, "flow_head")
        if not isinstance(it, torch.nn.Linear) or not isinstance(fh, torch.nn.Linear) or fh.in_features != it.out_features:
            fail("input_transform / flow_head", "not Linear(input -> hidden) and Linear(hidden -> output)")
        self.Din, self.D, self.Dout = it.in_features, it.out_features, fh.out_features
        D = self.D
        for attr, K in (("input_transform", self.Din), ("flow_head", D)):
            if K % 4:
                fail(attr, f"K = {K}: the fp32 GEMM takes K in multiples of 4")
        self.input_norm = r.ln(need(former, "input_norm"), "input_norm", self.Din)
        self.output_norm = r.ln(need(former, "output_norm"), "output_norm", D)
        self.input_transform = (f32(it.weight), _bias(it))
        # flow_head's rows are padded to a multiple of 4 with zeros: the [M, ld] result is handed on as its first Dout columns, without a copy
        self.ldo = (self.Dout + 3) // 4 * 4
        wf = torch.zeros(self.ldo, D, dtype=torch.float32, device=fh.weight.device)
        wf[:self.Dout] = fh.weight.detach().float()
        bf = torch.zeros(self.ldo, dtype=torch.float32, device=fh.weight.device)
        if fh.bias is not None:
            bf[:self.Dout] = fh.bias.detach().float()
        self.flow_head = (wf, bf)
        time_blocks = list(need(former, "time_blocks"))
        vt = getattr(former, "virual_tracks", None)                  # (the reference's spelling)
        self.nv = int(need(former, "num_virtual_tracks")) if vt is not None else 0
        if self.nv:
            if tuple(vt.shape) != (1, self.nv, 1, D):
                fail("virual_tracks", f"{tuple(vt.shape)}, not (1, {self.nv}, 1, {D})")
            self.virtual = f32(vt).reshape(self.nv, 1, D)
            sv, p2v, v2p = (list(need(former, a)) for a in ("space_virtual_blocks", "space_point2virtual_blocks", "space_virtual2point_blocks"))
            nt, ns = len(time_blocks), len(sv)
            # blocks.py:122: a space stage after time block i when i % (nt // ns) == 0, taking space blocks 0, 1, ... in turn
            if ns < 1 or nt < ns or len(p2v) != ns or len(v2p) != ns:
                fail("space_virtual_blocks", f"{ns} space blocks (point2virtual {len(p2v)}, virtual2point {len(v2p)}) for {nt} time blocks")
            self.every = nt // ns
            stages = (nt + self.every - 1) // self.every
            if stages > ns:
                fail("space_virtual_blocks", f"time depth {nt} / space depth {ns}: the loop (a stage every {self.every} blocks) would index space block "
                                             f"{stages - 1} of {ns}")
        else:
            self.virtual, self.every, sv, p2v, v2p = None, 1, [], [], []
        if not time_blocks:
            fail("time_blocks", "empty")
        self.time_blocks = [self._block(r, b, f"time_blocks[{i}]", False) for i, b in enumerate(time_blocks)]
        self.space_virtual_blocks = [self._block(r, b, f"space_virtual_blocks[{i}]", False) for i, b in enumerate(sv)]
        self.space_point2virtual_blocks = [self._block(r, b, f"space_point2virtual_blocks[{i}]", True) for i, b in enumerate(p2v)]
        self.space_virtual2point_blocks = [self._block(r, b, f"space_virtual2point_blocks[{i}]", True) for i, b in enumerate(v2p)]
        self.launches = 0

    def _block(self, r, blk, where, cross):
        D, fail, need = self.D, r.fail, r.need
        aname = where + (".cross_attn" if cross else ".attn")
        at = need(blk, "cross_attn" if cross else "attn", where)
        if not isinstance(at, torch.nn.MultiheadAttention):
            fail(aname, f"{type(at).__name__}: not a torch.nn.MultiheadAttention")
        if not at.batch_first:
            fail(aname + ".batch_first", "False")
        if not at._qkv_same_embed_dim or at.in_proj_weight is None:
            fail(aname + "._qkv_same_embed_dim", "False: separate q / k / v projection widths are not served")
        if at.dropout != 0:
            fail(aname + ".dropout", f"{at.dropout}: the kernel has no dropout")
        if at.bias_k is not None or at.bias_v is not None:
            fail(aname + ".bias_k", "set: no appended bias rows")
        if at.add_zero_attn:
            fail(aname + ".add_zero_attn", "True")
        if at.embed_dim != D:
            fail(aname + ".embed_dim", f"{at.embed_dim}, not the hidden size {D}")
        H = int(at.num_heads)
        if H < 1 or D % H:
            fail(aname + ".num_heads", f"{H} does not divide embed_dim {D}")
        hd = D // H
        if hd % 4 or not 4 <= hd <= 64:
            fail(aname + ".num_heads", f"{H}: head dimension {hd}; gd_attention_small_fwd serves multiples of 4 from 4 to 64")
        mlp = need(blk, "mlp", where)
        fc1, fc2 = need(mlp, "fc1", where + ".mlp"), need(mlp, "fc2", where + ".mlp")
        r.exact_gelu(getattr(mlp, "act", None), where + ".mlp.act")
        if not (isinstance(fc1, torch.nn.Linear) and isinstance(fc2, torch.nn.Linear)) or fc1.in_features != D or fc2.in_features != fc1.out_features or \
                fc2.out_features != D or fc1.out_features % 4:
            fail(where + ".mlp", f"fc1 / fc2 do not map {D} -> hidden (a multiple of 4) -> {D}")
        w, b = f32(at.in_proj_weight), _lin_bias(at.in_proj_bias, 3 * D, at.in_proj_weight)
        norm = lambda nm: r.ln(need(blk, nm, where), f"{where}.{nm}", D)
        p = dict(H=H, cross=cross, norm1=norm("norm1"), norm2=norm("norm2"), out=(f32(at.out_proj.weight), _bias(at.out_proj)),
                 fc1=(f32(fc1.weight), _bias(fc1)), fc2=(f32(fc2.weight), _bias(fc2)))
        if cross:
            p["norm_context"] = norm("norm_context")
            p["q"], p["kv"] = (w[:D].contiguous(), b[:D].contiguous()), (w[D:].contiguous(), b[D:].contiguous())
        else:
            p["qkv"] = (w, b)
        return p

    # ------------------------------------------------------------------------------------------------------------------------------
    def _to(self, device):
        if self.flow_head[0].device == device:
            return
        for n in ("input_norm", "output_norm", "input_transform", "flow_head", "virtual", "time_blocks", "space_virtual_blocks",
                  "space_point2virtual_blocks", "space_virtual2point_blocks"):
            setattr(self, n, to_device(getattr(self, n), device))

    def _ln(self, x, p):
        self.launches += 1
        return ops.layernorm_fwd(x, p[0], p[1], p[2], save_stats=False)[0]

    def _gemm(self, a, p, **kw):
        self.launches += 1
        return _linear(self.linear, a, p[0], p[1], **kw)

    def _attend(self, q, k, v, seq_q, seq_k, H):
        """q [rows_q, >= D], k, v [rows_k, >= D] (column blocks; equal row strides within each) under their sequence layouts -> o [rows_q, D]."""
        D = self.D
        G0, G1, Lq, r0, r1, rl = seq_q
        _, _, Lk, c0, c1, cl = seq_k
        view = lambda t, L, a, b, c: torch.as_strided(t, (G0, G1, L, D), (a * t.stride(0), b * t.stride(0), c * t.stride(0), 1), t.storage_offset())
        o = torch.empty(q.shape[0], D, dtype=torch.float32, device=q.device)
        self.launches += 1
        ops.attention_small_fwd(view(q, Lq, r0, r1, rl), view(k, Lk, c0, c1, cl), view(v, Lk, c0, c1, cl), G0, G1, Lq, Lk, H, out=view(o, Lq, r0, r1, rl))
        return o

    def _tail(self, p, xn, o, out, accumulate):
        x1 = self._gemm(o, p["out"], residual=xn)                                           # the residual is the NORMED x (modules.py:174-183)
        f = self._gemm(self._ln(x1, p["norm2"]), p["fc1"], act=1)
        return self._gemm(f, p["fc2"], residual=x1, out=out, accumulate=accumulate)

    def self_block(self, p, x, seq, out=None, accumulate=False):
        """AttnBlock.forward on the rows x [R, D] (contiguous) under the sequence layout `seq`; the result replaces x, or goes (added, with
        accumulate) to `out` [R, D]."""
        D = self.D
        xn = self._ln(x, p["norm1"])
        qkv = self._gemm(xn, p["qkv"])
        o = self._attend(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], seq, seq, p["H"])
        return self._tail(p, xn, o, x if out is None else out, accumulate)

    def cross_block(self, p, x, ctx, seq, seq_ctx, out=None, accumulate=False):
        """CrossAttnBlock.forward: the rows x [R, D] attend to the rows ctx [Rc, D]."""
        D = self.D
        xn = self._ln(x, p["norm1"])
        q = self._gemm(xn, p["q"])
        kv = self._gemm(self._ln(ctx, p["norm_context"]), p["kv"])
        o = self._attend(q, kv[:, :D], kv[:, D:], seq, seq_ctx, p["H"])
        return self._tail(p, xn, o, x if out is None else out, accumulate)

    @torch.no_grad()
    def __call__(self, x, mask=None):
        if mask is not None:
            raise GdHipError(f"FusedUpdateFormer: {self.name}: a mask is not served")
        if x.dim() != 4 or x.shape[3] != self.Din or not x.is_cuda or x.dtype != torch.float32:
            raise GdHipError(f"FusedUpdateFormer: {self.name}: x {tuple(x.shape)} {x.dtype} on {x.device} is not fp32 [B, N, S, {self.Din}] on the GPU")
        self._to(x.device)
        B, N, S, _ = x.shape
        D, nv, M = self.D, self.nv, B * N * S
        n = N + nv
        self.launches = 0
        fin = self._gemm(self._ln(x.reshape(M, self.Din), self.input_norm), self.input_transform).view(B, N * S, D)       # init_tokens; the result grows on it
        tok = torch.empty(B, n, S, D, dtype=torch.float32, device=x.device)
        tok[:, :N].copy_(fin.view(B, N, S, D))
        if nv:
            tok[:, N:].copy_(self.virtual.expand(nv, S, D))                                  # once per call
        self.launches += 2 if nv else 1
        rows = tok.view(B, n * S, D)
        pts, virt = rows[:, :N * S], rows[:, N * S:]
        seq_p, seq_v = (1, S, N, 0, 1, S), (1, S, nv, 0, 1, S)
        nt, j = len(self.time_blocks), 0
        for i, p in enumerate(self.time_blocks):
            space = nv > 0 and i % self.every == 0
            last = i == nt - 1
            if last and not space:                                                            # the virtual rows are dead: the point rows alone, onto fin
                for b in range(B):
                    self.self_block(p, pts[b], (N, 1, S, S, 0, 1), out=fin[b], accumulate=True)
                break
            self.self_block(p, tok.view(B * n * S, D), (B * n, 1, S, S, 0, 1))
            if space:
                for b in range(B):
                    self.cross_block(self.space_virtual2point_blocks[j], virt[b], pts[b], seq_v, seq_p)
                    self.self_block(self.space_virtual_blocks[j], virt[b], seq_v)
                    self.cross_block(self.space_point2virtual_blocks[j], pts[b], virt[b], seq_p, seq_v, out=fin[b] if last else None, accumulate=last)
                j += 1
        y = self._ln(fin.view(M, D), self.output_norm)
        delta = self._gemm(y, self.flow_head)
        return delta.view(B, N, S, self.ldo)[..., :self.Dout], None


class TrackState:
    """What one call carries from iteration to iteration.  coords [B, N, S, 2] (map cells) and track_feats [B, N, S, C] are in the loop's row order;
    `load` / `coords_bsn` / `feats_bsn` translate from and to the module's [B, S, N, .]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def load(self, coords_bsn=None, feats_bsn=None):
        if coords_bsn is not None:
            self.coords = coords_bsn.float().permute(0, 2, 1, 3).contiguous()
        if feats_bsn is not None:
            self.feats = feats_bsn.float().permute(0, 2, 1, 3).contiguous()
        return self

    @property
    def coords_bsn(self):
        return self.coords.permute(0, 2, 1, 3)

    @property
    def feats_bsn(self):
        return self.feats.permute(0, 2, 1, 3)


class FusedTracker:
    """FusedTracker(tracker).forward(query_points, fmaps, iters, ...) -> what the module's forward returns.  fp32 only (see the module docstring:
    a 16-bit mode is not offered).  The parameters are read and packed once, here, on whatever device the module is on (build it after loading the
    checkpoint); if that is not the device of the feature map handed to `begin` / `forward`, the packed copies are moved there on that call (`_to`).
    The user's `updateformer` is called as it stands and must itself live on the feature map's device; fused_updateformer=True (off by default) runs
    it as a FusedUpdateFormer instead, read and refused here like everything else.  linear="tokens" (off by default) runs the tracker's own linear
    layers (corr_mlp, ffeat_updater, the predictors) on gd_tokens_linear instead of gd_gemm_nt and hands the choice to the FusedUpdateFormer."""

    def __init__(self, tracker, name="tracker", fused_updateformer=False, *, linear="gemm_nt"):
        self.name = name
        self.linear = _linear_kind(linear, f"FusedTracker: {name}")
        r = Reader("FusedTracker", name)
        fail, need = r.fail, r.need
        C = int(need(tracker, "latent_dim"))
        if C != C_LATENT:
            fail("latent_dim", f"{C}: the tracker kernels serve {C_LATENT}")
        self.C, self.D = C, 3 * C + 4
        self.radius, self.levels = int(need(tracker, "corr_radius")), int(need(tracker, "corr_levels"))
        if not 0 <= self.radius <= MAX_RADIUS:
            fail("corr_radius", f"{self.radius}: gd_corr_sample serves 0 .. {MAX_RADIUS}")
        if not 1 <= self.levels <= MAX_LEVELS:
            fail("corr_levels", f"{self.levels}: gd_corr_sample serves 1 .. {MAX_LEVELS}")
        self.stride, self.max_scale = need(tracker, "stride"), float(need(tracker, "max_scale"))
        if self.max_scale == 0:
            fail("max_scale", "0")
        self.fmap_norm = r.ln(need(tracker, "fmap_norm"), "fmap_norm", C)
        gn = need(tracker, "ffeat_norm")
        if not (isinstance(gn, torch.nn.GroupNorm) and gn.affine and gn.num_groups == 1 and gn.num_channels == C):
            fail("ffeat_norm", f"not an affine GroupNorm(1, {C})")
        self.ffeat_norm = (f32(gn.weight), f32(gn.bias), float(gn.eps))
        # corr_mlp: Linear(levels * (2r+1)^2 -> hidden), exact GELU, Linear(hidden -> C); K is padded to the fp32 GEMM's 128-byte K steps
        mlp = need(tracker, "corr_mlp")
        fc1, fc2 = need(mlp, "fc1", "corr_mlp"), need(mlp, "fc2", "corr_mlp")
        r.exact_gelu(getattr(mlp, "act", None), "corr_mlp.act")
        K = self.levels * (2 * self.radius + 1) ** 2
        if not (isinstance(fc1, torch.nn.Linear) and isinstance(fc2, torch.nn.Linear)) or fc1.in_features != K or fc2.in_features != fc1.out_features or \
                fc2.out_features != C:
            fail("corr_mlp", f"fc1 / fc2 do not map {K} -> hidden -> {C}")
        self.kpad = (K + 31) // 32 * 32
        self._gemm_ok("corr_mlp.fc1", self.kpad, fail)
        self._gemm_ok("corr_mlp.fc2", fc2.in_features, fail)
        w1 = torch.zeros(fc1.out_features, self.kpad, dtype=torch.float32, device=fc1.weight.device)
        w1[:, :K] = fc1.weight.detach().float()
        self.corr_mlp = (w1, _bias(fc1), f32(fc2.weight), _bias(fc2))
        up = need(tracker, "ffeat_updater")
        mods = list(up) if isinstance(up, torch.nn.Sequential) else []
        if len(mods) != 2 or not isinstance(mods[0], torch.nn.Linear) or mods[0].in_features != C or mods[0].out_features != C:
            fail("ffeat_updater", f"not Sequential(Linear({C}, {C}), GELU)")
        r.exact_gelu(mods[1], "ffeat_updater[1]")
        self._gemm_ok("ffeat_updater[0]", C, fail)
        self.ffeat_updater = (f32(mods[0].weight), _bias(mods[0]))
        self.updateformer = need(tracker, "updateformer")
        if fused_updateformer:
            self.updateformer = FusedUpdateFormer(self.updateformer, name=f"{name}.updateformer", linear=linear)
            if self.updateformer.Din != self.D or self.updateformer.Dout != C + 2:
                fail("updateformer", f"maps {self.updateformer.Din} -> {self.updateformer.Dout}, not {self.D} -> {C + 2}")
        qrt = need(tracker, "query_ref_token")
        if tuple(qrt.shape) != (1, 2, self.D):
            fail("query_ref_token", f"{tuple(qrt.shape)}, not (1, 2, {self.D})")
        self.qrt = f32(qrt).reshape(2, self.D)
        self.predict_conf = bool(getattr(tracker, "predict_conf", False))
        heads = [("vis_predictor", need(tracker, "vis_predictor"))]
        if self.predict_conf:
            if getattr(tracker, "conf_predictor", None) is None:
                fail("conf_predictor", "missing while predict_conf is set")
            heads.append(("conf_predictor", tracker.conf_predictor))
        # the one-output predictors share ONE GEMM: their weights are rows 0 (vis) and 1 (conf) of an [8, C] matrix, the other rows zero
        wp = torch.zeros(8, C, dtype=torch.float32, device=self.qrt.device)
        bp = torch.zeros(8, dtype=torch.float32, device=self.qrt.device)
        for i, (attr, m) in enumerate(heads):
            lin = m[0] if isinstance(m, torch.nn.Sequential) and len(m) == 1 else m
            if not isinstance(lin, torch.nn.Linear) or lin.in_features != C or lin.out_features != 1:
                fail(attr, f"not a Linear({C}, 1) (alone or as the only entry of a Sequential)")
            wp[i] = lin.weight.detach().float()[0]
            if lin.bias is not None:
                bp[i] = lin.bias.detach().float()[0]
        self.predictors = (wp, bp)
        self._omega = {}

    _TENSORS = ("fmap_norm", "ffeat_norm", "corr_mlp", "ffeat_updater", "predictors")

    def _to(self, device):
        """The packed parameters follow the feature map's device: a tracker read while the teacher was still on the host is moved on its first call."""
        if self.qrt.device != device:
            self.qrt = self.qrt.to(device)
            for n in self._TENSORS:
                setattr(self, n, to_device(getattr(self, n), device))

    @staticmethod
    def _gemm_ok(attr, K, fail):
        """gd_gemm_nt takes fp32 operands whose K and row strides are multiples of 16 bytes: refused here, at construction, not in the loop."""
        if K % 4:
            fail(attr, f"K = {K}: the fp32 GEMM takes K in multiples of 4")

    # ------------------------------------------------------------------------------------------------------------------------------
    def _channel_last(self, fmaps, fmaps_cl, pitch):
        """-> (map [B*S, H, pitch, C] contiguous fp32, B, S, H, W, pitch).  fmaps: NCHW [B, S, C, H, W].  fmaps_cl: [B, S, H, W, C], either contiguous
        or the data columns of a pitched buffer (strides (S*H*pitch*C, H*pitch*C, pitch*C, C, 1), e.g. FusedDPTHead(..., channel_last=True))."""
        C = self.C
        if (fmaps is None) == (fmaps_cl is None):
            raise GdHipError("FusedTracker: give fmaps (NCHW) or fmaps_cl (channel-last), not both")
        if fmaps is not None:
            if fmaps.dim() != 5 or fmaps.shape[2] != C or not fmaps.is_cuda:
                raise GdHipError(f"FusedTracker: fmaps {tuple(fmaps.shape)} on {fmaps.device} is not [B, S, {C}, H, W] on the GPU")
            B, S, _, H, W = fmaps.shape
            return fmaps.float().permute(0, 1, 3, 4, 2).contiguous().view(B * S, H, W, C), B, S, H, W, W
        t = fmaps_cl
        if t.dim() != 5 or t.shape[4] != C or not t.is_cuda or t.dtype != torch.float32:
            raise GdHipError(f"FusedTracker: fmaps_cl {tuple(t.shape)} {t.dtype} on {t.device} is not fp32 [B, S, H, W, {C}] on the GPU")
        B, S, H, W, _ = t.shape
        p = self.pitch_of(t, pitch)
        if p == W:
            return torch.as_strided(t, (B * S, H, W, C), (H * W * C, W * C, C, 1)), B, S, H, W, W
        try:
            return torch.as_strided(t, (B * S, H, p, C), (H * p * C, p * C, C, 1)), B, S, H, W, p
        except RuntimeError as e:
            raise GdHipError(f"FusedTracker: fmaps_cl does not sit in a buffer of whole pitched rows (pitch {p}): {e}")

    @staticmethod
    def pitch_of(t, pitch=None):
        """The pitch (cells per map row in memory) of a channel-last map t [B, S, H, W, C]: `pitch` when given, else read off the row stride.  Raises unless
        t's strides are those of [B, S, H, pitch, C] rows; the stride of a dimension of size 1 is arbitrary and is not compared."""
        B, S, H, W, C = t.shape
        p = int(pitch) if pitch is not None else (t.stride(2) // C if H > 1 else W)
        want = (S * H * p * C, H * p * C, p * C, C, 1)
        if p < W or any(n > 1 and st != w for n, st, w in zip(t.shape, t.stride(), want)):
            raise GdHipError(f"FusedTracker: fmaps_cl strides {tuple(t.stride())} are not those of [B, S, H, pitch = {p}, {C}] rows")
        return p

    @torch.no_grad()
    def begin(self, query_points, fmaps=None, down_ratio=1, *, fmaps_cl=None, pitch=None):
        """-> the TrackState before the first iteration (base_track_predictor.py:88-118)."""
        fm, B, S, H, W, p = self._channel_last(fmaps, fmaps_cl, pitch)
        self._to(fm.device)
        if query_points.dim() != 3 or query_points.shape[0] != B or query_points.shape[2] != 2:
            raise GdHipError(f"FusedTracker: query_points {tuple(query_points.shape)} is not [B = {B}, N, 2]")
        check_levels(H, W, self.levels)
        C, N = self.C, query_points.shape[1]
        q = query_points.to(fm.device, torch.float32)
        if down_ratio > 1:
            q = q / float(down_ratio)
        q = (q / float(self.stride)).contiguous()
        g, b, eps = self.fmap_norm
        fm = ops.layernorm_fwd(fm.view(B * S * H * p, C), g, b, eps, save_stats=False)[0].view(B * S, H, p, C)       # separator rows: finite, never read
        pyramid = ops.corr_pyramid(fm, W, self.levels)
        qfeat = ops.points_bilinear(fm, W, q, frame_step=S)
        key = str(fm.device)
        if key not in self._omega:
            self._omega[key] = ops.track_pos_omega(self.D, fm.device)
        return TrackState(B=B, S=S, N=N, H=H, W=W, pyramid=pyramid, query_feat=qfeat,
                          coords=q[:, :, None, :].expand(B, N, S, 2).contiguous(), feats=qfeat[:, :, None, :].expand(B, N, S, C).contiguous(),
                          pos=ops.track_pos_embed(q.view(B * N, 2), H, W, self.D, self._omega[key]),
                          mul1=float(self.stride), mul2=float(down_ratio) if down_ratio > 1 else 1.0)

    @torch.no_grad()
    def step(self, st):
        """One iteration (base_track_predictor.py:123-192): updates st.coords / st.feats, -> the predicted coordinates [B, S, N, 2] at image scale."""
        B, S, N, C = st.B, st.S, st.N, self.C
        M = B * N * S
        corr = ops.corr_sample(st.pyramid, st.feats, st.coords, self.radius, ld=self.kpad)
        st.corr = corr
        w1, b1, w2, b2 = self.corr_mlp
        c = _linear(self.linear, _linear(self.linear, corr.view(M, self.kpad), w1, b1, act=1), w2, b2)
        x = ops.track_assemble(st.coords, c.view(B, S, N, C), st.feats, st.pos, self.qrt, self.max_scale)
        delta = self.updateformer(x)
        delta = delta[0] if isinstance(delta, (tuple, list)) else delta
        if tuple(delta.shape) != (B, N, S, C + 2):
            raise GdHipError(f"FusedTracker: {self.name}.updateformer returned {tuple(delta.shape)}, not {(B, N, S, C + 2)}")
        pred, dfeat = ops.track_update(delta.float(), st.coords, st.mul1, st.mul2)
        g, b, eps = self.ffeat_norm
        y = ops.layernorm_fwd(dfeat, g, b, eps, save_stats=False)[0]
        wu, bu = self.ffeat_updater
        st.feats = _linear(self.linear, y, wu, bu, act=1, residual=st.feats.view(M, C)).view(B, N, S, C)
        return pred

    @torch.no_grad()
    def finish(self, st, apply_sigmoid=True):
        """-> (vis [B, S, N], conf [B, S, N] or None) (base_track_predictor.py:194-204)."""
        B, S, N, C = st.B, st.S, st.N, self.C
        o = _linear(self.linear, st.feats.view(B * N * S, C), self.predictors[0], self.predictors[1]).view(B, N, S, 8)
        vis = o[..., 0].permute(0, 2, 1)
        conf = o[..., 1].permute(0, 2, 1) if self.predict_conf else None
        if apply_sigmoid:
            vis, conf = torch.sigmoid(vis), (torch.sigmoid(conf) if conf is not None else None)
        return vis, conf

    @torch.no_grad()
    def forward(self, query_points, fmaps=None, iters=6, return_feat=False, down_ratio=1, apply_sigmoid=True, *, fmaps_cl=None, pitch=None):
        """Same arguments and result as the module's forward: ([iters x coords [B, S, N, 2] at image scale], vis, conf), or with return_feat
        (coords, vis, track_feats [B, S, N, C], query_track_feat [B, N, C], conf).  fmaps_cl / pitch: the channel-last map (see _channel_last)."""
        st = self.begin(query_points, fmaps, down_ratio, fmaps_cl=fmaps_cl, pitch=pitch)
        preds = [self.step(st) for _ in range(iters)]
        vis, conf = self.finish(st, apply_sigmoid)
        if return_feat:
            return preds, vis, st.feats_bsn, st.query_feat, conf
        return preds, vis, conf

    __call__ = forward
