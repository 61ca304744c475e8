"""Reading a user's teacher module for the fused paths (teacher_blocks, teacher_heads, teacher_tracker): the modules are duck-typed on the
reference's attribute names, their parameters are packed once, and what the kernels do not serve is refused with
    <class>: <module name>.<dotted.attribute.path>: <why>
A Reader carries the first two parts; everything a fused class asks of a module goes through it."""
import torch

from ._lib import GdHipError


def f32(t):
    return None if t is None else t.detach().float().contiguous()


def to_device(pack, device):
    """A packed parameter set (a tensor, or tuples / lists / dicts of tensors and plain values) with every tensor on `device`."""
    if torch.is_tensor(pack):
        return pack.to(device)
    if isinstance(pack, (tuple, list)):
        return type(pack)(to_device(v, device) for v in pack)
    if isinstance(pack, dict):
        return {k: to_device(v, device) for k, v in pack.items()}
    return pack


class Reader:
    def __init__(self, who, name):
        self.who, self.name = who, name

    def fail(self, attr, why):
        raise GdHipError(f"{self.who}: {self.name}.{attr}: {why}")

    def need(self, obj, attr, where="", none_ok=False):
        """obj.attr, `where` being obj's own path under the module.  Missing: the attribute is absent, or None unless none_ok."""
        v = getattr(obj, attr, self)
        if v is self or (v is None and not none_ok):
            self.fail(f"{where}.{attr}" if where else attr, "missing")
        return v

    def ln(self, mod, attr, width=None):
        """-> (weight, bias, eps) of an affine LayerNorm over `width` columns (None: any one width), vectors fp32.  A LayerNorm(bias=False) is
        refused: gd_layernorm_fwd and gd_qk_norm_rope read beta wherever they read gamma.  (The refusal repeats the attribute's last name,
        '<path>.norm: .norm is not ...', the wording the host tests of the embedder's final norm look for.)"""
        if not (isinstance(mod, torch.nn.LayerNorm) and mod.elementwise_affine and mod.bias is not None and len(mod.normalized_shape) == 1
                and width in (None, mod.normalized_shape[0])):
            self.fail(attr, f".{attr.rsplit('.', 1)[-1]} is not an affine LayerNorm({'width' if width is None else width}) with a bias")
        return f32(mod.weight), f32(mod.bias), float(mod.eps)

    def linear(self, mod, attr, k=None, n=None, cast=f32):
        """-> (cast(weight), fp32 bias or None) of a Linear(k -> n); None: any."""
        if not isinstance(mod, torch.nn.Linear) or k not in (None, mod.in_features) or n not in (None, mod.out_features):
            self.fail(attr, f"not a Linear({'.' if k is None else k} -> {'.' if n is None else n})")
        return cast(mod.weight), f32(mod.bias)

    def exact_gelu(self, mod, attr, allow_none=False):
        """allow_none: a layout without the attribute calls F.gelu itself (vggt/layers/mlp.py keeps act_layer())."""
        if mod is None and allow_none:
            return
        if not (isinstance(mod, torch.nn.GELU) and getattr(mod, "approximate", "none") == "none"):
            self.fail(attr, f"{mod}: the GEMM epilogue serves exact (erf) GELU")

    def no_dropout(self, mod, attr):
        p = float(getattr(mod, "p", 0.0)) if mod is not None else 0.0
        if p != 0.0 and getattr(mod, "training", False):
            self.fail(attr, f"p = {p} in training mode: the kernels have no dropout")
