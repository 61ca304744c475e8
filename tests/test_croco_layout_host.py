"""CPU: the test-owned MASt3R module tree (tests/croco_layout.py) against fixture G25 — what the REFERENCE's own Block / DecoderBlock /
`_decoder` / `forward` returned with the deterministic weights of `fill_params` (tools/make_golden_g25.py) —, the one-head head-mean identity
that FusedCroCoBlocks.decode's map contract rests on, and the argument guards of gd_cross_attention_fwd (no GPU: every call stops at a guard)."""
import ctypes

import pytest
import torch
import torch.nn as nn

import croco_layout as CL
from test_teacher_runner_ref import fill_params


@pytest.fixture(scope="module")
def layout_run():
    """(golden, encoder-block outputs, decoder outputs, per-head maps 1 / 2, tgt_attn_map) of the layout in float32 on the fixture's inputs."""
    from conftest import load_golden
    g = load_golden("g25_mast3r_blocks")
    m = CL.CrocoLayout(**CL.CFG).eval()
    assert CL.param_layout(m) == g["param_layout"]            # the name order fill_params depends on
    fill_params(m)
    with torch.no_grad():
        enc = [m.encode_blocks(g["x1"], g["pos1"]), m.encode_blocks(g["x2"], g["pos2"])]
        f1, f2 = m.enc_norm(enc[0]), m.enc_norm(enc[1])
        outs, maps1, maps2 = m._decoder(f1, g["pos1"], f2, g["pos2"])
        _, tgt = m.target(f1, g["pos1"], f2, g["pos2"])
    return g, m, enc, outs, maps1, maps2, tgt


def test_layout_reproduces_the_reference_blocks(layout_run):
    g, m, enc, outs, maps1, maps2, tgt = layout_run
    x1, x2 = CL.seeded_inputs()[0], CL.seeded_inputs()[2]
    assert torch.equal(x1, g["x1"]) and torch.equal(x2, g["x2"])
    assert torch.equal(CL.grid_positions(CL.B, *CL.GRID1), g["pos1"]) and torch.equal(CL.grid_positions(CL.B, *CL.GRID2), g["pos2"])

    def close(got, want, what):
        e, bound = float((got - want).abs().max()), 1e-4 * float(want.abs().max())
        assert got.shape == want.shape and e <= bound, (what, e, bound)
    close(enc[0], g["enc_1"], "enc_1")
    close(enc[1], g["enc_2"], "enc_2")
    assert len(outs[0]) == len(outs[1]) == CL.CFG["dec_depth"] + 1
    for v in range(2):
        for i, t in enumerate(outs[v]):
            close(t, g[f"out{v + 1}_{i}"], f"out{v + 1}_{i}")
    for l in range(CL.CFG["dec_depth"]):
        assert maps1[l].shape == (2, 2, 21, 20) and maps2[l].shape == (2, 2, 20, 21)
        close(maps1[l].mean(dim=1, keepdim=True), g[f"camap1_{l}"], f"camap1_{l}")
        close(maps2[l].mean(dim=1, keepdim=True), g[f"camap2_{l}"], f"camap2_{l}")
    assert tgt.shape == (2, 21, 20) and float((tgt - g["tgt_attn_map"]).abs().max()) <= 1e-6


@pytest.mark.parametrize("reciprocity", [True, False])
def test_one_head_head_means_serve_both_consumers(layout_run, reciprocity):
    """Both consumers of the decoder's score maps take .mean(dim=1) first, so [B, 1, Nq, Nk] head means give what the per-head maps give."""
    import gd_amd  # noqa: F401
    from gd_amd import teacher_glue as tg
    g, m, enc, outs, maps1, maps2, tgt = layout_run
    mean1, mean2 = [t.mean(dim=1, keepdim=True) for t in maps1], [t.mean(dim=1, keepdim=True) for t in maps2]
    assert mean1[0].shape == (2, 1, 21, 20) and mean2[0].shape == (2, 1, 20, 21)
    f1, f2 = m.enc_norm(enc[0]), m.enc_norm(enc[1])
    m.reciprocity = reciprocity
    try:
        with torch.no_grad():
            _, full = m.target(f1, g["pos1"], f2, g["pos2"])
            _, one = m.target(f1, g["pos1"], f2, g["pos2"], decoder=lambda *a: (outs, mean1, mean2))
    finally:
        m.reciprocity = CL.CFG["reciprocity"]
    assert float((full - one).abs().max()) <= 1e-6
    if reciprocity:
        assert float((full - tgt).abs().max()) <= 1e-6
    a, b = tg.mast3r_recip_logits(maps1, maps2), tg.mast3r_recip_logits(mean1, mean2)
    assert a.shape == b.shape == (2, 2, 21, 20) and float((a - b).abs().max()) <= 1e-6


def _call(L, B, Nq, Nk, H, hd, ldq, ldkv, dtype=0):
    return L.gd_cross_attention_fwd(None, None, None, None, B, Nq, Nk, H, hd, ldq, ldkv, ctypes.c_float(0.125), dtype, None)


def test_cross_attention_argument_guards():
    """Null pointers, no GPU: every one of these stops at a guard before any HIP call."""
    from gd_amd import _lib
    L = _lib.lib()
    err = lambda: L.gd_last_error().decode()
    assert _call(L, 1, 16, 16, 2, 32, 64, 128) != 0 and "head_dim" in err()
    assert _call(L, 1, 16, 16, 2, 64, 64, 256) != 0 and "ldq" in err() and "stride" in err()            # ldq < H * 64
    assert _call(L, 1, 16, 16, 2, 64, 128, 192) != 0 and "ldkv" in err() and "stride" in err()          # ldkv < 2 * H * 64
    assert _call(L, 1, 16, 0, 2, 64, 128, 256) != 0 and "bad shape" in err() and "Nk=0" in err()
    assert _call(L, 1, 1 << 20, 16, 16, 64, 1024, 2048, _lib.BF16) != 0 and "2^31" in err() and "q rows" in err()
    assert _call(L, 1, 16, 1 << 20, 16, 64, 1024, 2048, _lib.BF16) != 0 and "2^31" in err() and "kv rows" in err()
    assert _call(L, 1, 16, 16, 2, 64, 130, 256, _lib.BF16) != 0 and "16 bytes" in err()               # 260-byte rows
    assert _call(L, 1, 16, 16, 2, 64, 128, 256, 7) != 0 and "dtype" in err()


# ----------------------------------------------------------------------------------------------------------------------------------
# FusedCroCoBlocks: what it refuses, at construction, naming the block and the attribute (no device)
# ----------------------------------------------------------------------------------------------------------------------------------
def _edit(path, value):
    def edit(m):
        obj, names = m, path.split(".")
        for n in names[:-1]:
            obj = obj[int(n)] if n.isdigit() else getattr(obj, n)
        setattr(obj, names[-1], value)
    return edit


def _drop(path):
    def edit(m):
        obj, names = m, path.split(".")
        for n in names[:-1]:
            obj = obj[int(n)] if n.isdigit() else getattr(obj, n)
        delattr(obj, names[-1])
    return edit


CROCO_REFUSALS = [
    ({}, _drop("enc_blocks.0.attn"), r"enc_blocks\[0\].*attn"),
    ({}, _drop("dec_blocks.1.mlp"), r"dec_blocks\[1\].*mlp"),
    ({}, _drop("enc_blocks.1.norm1"), r"enc_blocks\[1\].*norm1"),
    ({}, _drop("dec_blocks2.0.cross_attn"), r"dec_blocks2\[0\].*cross_attn"),
    ({}, _drop("dec_blocks.0.norm_y"), r"dec_blocks\[0\].*norm_y"),
    ({}, _drop("dec_blocks.0.cross_attn.projq"), r"dec_blocks\[0\].*cross_attn.*projq"),
    ({}, _drop("enc_blocks.0.mlp.fc1"), r"enc_blocks\[0\].*fc1"),
    (dict(enc_heads=6), None, r"enc_blocks\[0\].*head dim 32"),
    ({}, _edit("dec_blocks.0.attn.scale", 0.2), r"dec_blocks\[0\].*attn\.scale"),
    ({}, _edit("dec_blocks.1.cross_attn.scale", 0.2), r"dec_blocks\[1\].*cross_attn\.scale"),
    ({}, _edit("enc_blocks.1.attn.rope", None), r"enc_blocks\[1\].*attn\.rope"),
    ({}, _edit("dec_blocks2.1.cross_attn.rope", None), r"dec_blocks2\[1\].*cross_attn\.rope"),
    ({}, _edit("enc_blocks.0.mlp.act", nn.GELU(approximate="tanh")), r"enc_blocks\[0\].*mlp\.act"),
    ({}, _edit("dec_blocks2.1.mlp.act", nn.ReLU()), r"dec_blocks2\[1\].*mlp\.act"),
    ({}, _edit("dec_blocks.0.norm3", nn.LayerNorm(128, elementwise_affine=False)), r"dec_blocks\[0\].*norm3"),
    ({}, _edit("dec_blocks.1.norm2", nn.LayerNorm(64)), r"dec_blocks\[1\].*norm2"),
    ({}, _edit("enc_blocks.1.norm2", nn.Identity()), r"enc_blocks\[1\].*norm2"),
    ({}, _edit("dec_blocks2.0.norm_y", nn.BatchNorm1d(128)), r"dec_blocks2\[0\].*norm_y"),
    ({}, _edit("dec_blocks.0.cross_attn.num_heads", 1), r"dec_blocks\[0\].*cross_attn.*head dim 128"),
    ({}, _edit("dec_blocks.1.cross_attn.rope", CL.DeviceRope2D(10.0)), r"dec_blocks\[1\].*cross_attn.*RoPE base"),
    ({}, _edit("dec_blocks.0.cross_attn.projv", nn.Linear(128, 128, bias=False)), r"dec_blocks\[0\].*cross_attn\.projk"),
    (dict(dec_depth2=1), None, r"dec_blocks.*dec_blocks2"),
    (dict(dec_depth=0), None, r"dec_blocks"),
    ({}, _edit("decoder_embed", nn.Identity()), r"decoder_embed"),
    ({}, _edit("decoder_embed", nn.Linear(192, 64)), r"dec_blocks\[0\].*width 128"),
    ({}, _drop("dec_norm"), r"dec_norm"),
    ({}, _edit("dec_norm", nn.LayerNorm(128, elementwise_affine=False)), r"dec_norm"),
    ({}, _drop("enc_blocks"), r"enc_blocks"),
]


@pytest.mark.parametrize("case", range(len(CROCO_REFUSALS)))
def test_fused_croco_blocks_refuse_what_the_kernels_do_not_serve(case):
    import gd_amd  # noqa: F401
    from gd_amd._lib import GdHipError
    from gd_amd.teacher_blocks import FusedCroCoBlocks
    over, edit, match = CROCO_REFUSALS[case]
    m = CL.CrocoLayout(**dict(CL.CFG, **over)).eval()
    if edit is not None:
        FusedCroCoBlocks(m)                                                              # accepted as it stands
        edit(m)
    with pytest.raises(GdHipError, match=match) as e:
        FusedCroCoBlocks(m)
    print(e.value)
    assert str(e.value).startswith("FusedCroCoBlocks: ")
    with pytest.raises(GdHipError, match="dtype"):
        FusedCroCoBlocks(CL.CrocoLayout(**CL.CFG), dtype=torch.float16)


def test_fused_croco_blocks_accept_identity_norm_y_and_biasless_cross_projections():
    import gd_amd  # noqa: F401
    from gd_amd.teacher_blocks import FusedCroCoBlocks
    m = CL.CrocoLayout(**CL.CFG).eval()
    m.dec_blocks[1].norm_y = nn.Identity()                                               # norm_mem=False
    ca = m.dec_blocks2[0].cross_attn
    ca.projk, ca.projv = nn.Linear(128, 128, bias=False), nn.Linear(128, 128, bias=False)
    f = FusedCroCoBlocks(m, dtype=torch.bfloat16)
    assert f.dec1[1].ny is None and f.dec1[0].ny is not None and f.dec2[0].bkv is None
    p = f.dec1[0]
    assert p.wkv.shape == (256, 128) and p.wkv.dtype == torch.bfloat16 and p.bkv.shape == (256,) and p.bkv.dtype == torch.float32
    assert torch.equal(p.wkv[128:], m.dec_blocks[0].cross_attn.projv.weight.detach().to(torch.bfloat16))
    assert (p.H, p.C, p.base) == (2, 128, 100.0) and (f.enc[0].H, f.enc[0].C) == (3, 192)
