"""Test-owned layout of the VGGT teacher's camera head: a module tree with the reference CameraHead's parameter names and arithmetic (iterative
refinement of the camera token through an adaLN-modulated transformer trunk), and a restatement of the pose decoding.  tools/make_golden_g30.py
asserts that this layout reproduces the reference's own module, parameter layout included, before it writes fixture G30; the tests run the layout
(fp32 and fp64) as the yardstick of teacher_heads.FusedCameraHead."""
import torch
import torch.nn as nn
import torch.nn.functional as F

# the two tiny configurations: (dim_in, heads, depth); the second has the teacher's head dimension, 128
CONFIGS = {"d64": dict(dim_in=64, num_heads=4, trunk_depth=2), "d256": dict(dim_in=256, num_heads=2, trunk_depth=1)}
SHAPES = [(1, 2), (2, 3)]               # (B, S) of the fixture's camera-token inputs
PATCH_TOKENS = 3                        # rows behind the camera row in the fixture's token tensors
IMAGE_HW = (42, 70)
ACTS = {"linear": lambda t: t, "inv_log": lambda t: torch.sign(t) * torch.expm1(t.abs()), "exp": torch.exp, "relu": F.relu}


class _Scale(nn.Module):
    def __init__(self, dim, init):
        super().__init__()
        self.gamma = nn.Parameter(init * torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class _Attention(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads, self.head_dim = num_heads, dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.qkv, self.proj = nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.q_norm, self.k_norm = nn.Identity(), nn.Identity()
        self.attn_drop, self.proj_drop = nn.Dropout(0.0), nn.Dropout(0.0)
        self.rope = None

    def forward(self, x, pos=None):
        B, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
        a = ((q * self.scale) @ k.transpose(-2, -1)).softmax(dim=-1)
        return self.proj((a @ v).transpose(1, 2).reshape(B, N, C))


class _Mlp(nn.Module):
    def __init__(self, dim, hidden, out):
        super().__init__()
        self.fc1, self.act, self.fc2, self.drop = nn.Linear(dim, hidden), nn.GELU(), nn.Linear(hidden, out), nn.Dropout(0.0)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class _Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, init_values):
        super().__init__()
        self.norm1, self.attn, self.ls1 = nn.LayerNorm(dim), _Attention(dim, num_heads), _Scale(dim, init_values)
        self.norm2, self.mlp, self.ls2 = nn.LayerNorm(dim), _Mlp(dim, int(dim * mlp_ratio), dim), _Scale(dim, init_values)

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


class CameraHeadLayout(nn.Module):
    def __init__(self, dim_in=2048, trunk_depth=4, num_heads=16, mlp_ratio=4, init_values=0.01, trans_act="linear", quat_act="linear", fl_act="relu"):
        super().__init__()
        self.target_dim, self.trunk_depth = 9, trunk_depth
        self.trans_act, self.quat_act, self.fl_act = trans_act, quat_act, fl_act
        self.trunk = nn.Sequential(*[_Block(dim_in, num_heads, mlp_ratio, init_values) for _ in range(trunk_depth)])
        self.token_norm, self.trunk_norm = nn.LayerNorm(dim_in), nn.LayerNorm(dim_in)
        self.empty_pose_tokens = nn.Parameter(torch.zeros(1, 1, 9))
        self.embed_pose = nn.Linear(9, dim_in)
        self.poseLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(dim_in, 3 * dim_in))
        self.adaln_norm = nn.LayerNorm(dim_in, elementwise_affine=False, eps=1e-6)
        self.pose_branch = _Mlp(dim_in, dim_in // 2, 9)

    def activate(self, raw):
        return torch.cat([ACTS[self.trans_act](raw[..., :3]), ACTS[self.quat_act](raw[..., 3:7]), ACTS[self.fl_act](raw[..., 7:])], dim=-1)

    def forward(self, aggregated_tokens_list, num_iterations=4):
        tok = self.token_norm(aggregated_tokens_list[-1][:, :, 0])
        B, S, _ = tok.shape
        raw, out = None, []
        for _ in range(num_iterations):
            cond = self.embed_pose(self.empty_pose_tokens.expand(B, S, -1) if raw is None else raw)
            shift, scale, gate = self.poseLN_modulation(cond).chunk(3, dim=-1)
            x = self.trunk(gate * (self.adaln_norm(tok) * (1 + scale) + shift) + tok)
            delta = self.pose_branch(self.trunk_norm(x))
            raw = delta if raw is None else raw + delta
            out.append(self.activate(raw))
        return out


def decode_pose(enc, image_hw):
    """enc [..., 9] = translation | scalar-last quaternion | (fov_h, fov_w) -> (extrinsic [..., 3, 4], intrinsic [..., 3, 3]) in enc's dtype."""
    H, W = image_hw
    t, (i, j, k, r) = enc[..., :3], enc[..., 3:7].unbind(-1)
    s2 = 2.0 / (enc[..., 3:7] ** 2).sum(-1)
    R = torch.stack([1 - s2 * (j * j + k * k), s2 * (i * j - k * r), s2 * (i * k + j * r),
                     s2 * (i * j + k * r), 1 - s2 * (i * i + k * k), s2 * (j * k - i * r),
                     s2 * (i * k - j * r), s2 * (j * k + i * r), 1 - s2 * (i * i + j * j)], dim=-1).reshape(enc.shape[:-1] + (3, 3))
    K = torch.zeros(enc.shape[:-1] + (3, 3), dtype=enc.dtype, device=enc.device)
    K[..., 0, 0] = (W / 2.0) / torch.tan(enc[..., 8] / 2.0)
    K[..., 1, 1] = (H / 2.0) / torch.tan(enc[..., 7] / 2.0)
    K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = W / 2, H / 2, 1.0
    return torch.cat([R, t[..., None]], dim=-1), K


def fill_head(m):
    """fill_params' deterministic weights, then the pose branch conditioned so that the decoded cameras are well defined in every iteration: its
    output weights a tenth as large, + 1 on the quaternion's scalar part and + 0.4 rad on both fields of view per iteration (|q| stays away from 0
    and the fields of view inside (0, pi), away from tan's pole and from relu's corner).  The fixture's generator fills the reference's module the
    same way."""
    from test_teacher_runner_ref import fill_params
    fill_params(m)
    with torch.no_grad():
        m.pose_branch.fc2.weight.mul_(0.1)
        m.pose_branch.fc2.bias[6] += 1.0
        m.pose_branch.fc2.bias[7:] += 0.4
    return m


def make_head(cfg, **over):
    return fill_head(CameraHeadLayout(**dict(CONFIGS[cfg], **over)).eval())


def attach_camera_head(vggt, head):
    """Put a real camera head in place of dpt_layout.TinyVGGT's stub METHOD: an instance attribute, which shadows the class's function (a registered
    submodule would not: attribute lookup finds the class's function first).  The head is therefore moved between devices by the caller."""
    vggt.__dict__["camera_head"] = head
    return vggt


def seeded_tokens(cfg, B, S):
    """tokens_list as the aggregator hands it over: only the last entry is read, [B, S, 1 + PATCH_TOKENS, dim_in]."""
    g = torch.Generator().manual_seed(3000 + 100 * B + 10 * S + CONFIGS[cfg]["dim_in"])
    return [torch.randn(B, S, 1 + PATCH_TOKENS, CONFIGS[cfg]["dim_in"], generator=g)]


def param_layout(m):
    return ",".join(f"{n}:{'x'.join(map(str, p.shape))}" for n, p in sorted(m.named_parameters()))
