"""fp64 restatement of gd_attention_small_fwd (csrc/small_attn.hip) and its per-element bound, in the manner of tests/rowwise_ref64.py and
tests/track_corr_ref64.py: the truth is computed in fp64 from the SAME fp32 inputs, addressed cell by cell exactly as the C ABI states it
(row i of sequence (g0, g1) at base + g0 * s0 + g1 * s1 + i * ld, head h in columns [h * hd, (h + 1) * hd)), and the bound follows the kernel's order of
operations; nothing in it is fitted to the kernel's output.

The bound.  U = 2^-24 (fp32 round to nearest), s_j = scale q . k_j, A = max_j scale sum_d |q_d k_jd|, m = max_j s_j, p_j = exp(s_j - m),
x = max_j |s_j - m|.  The kernel computes, per output element (row i, column c of head h):

  scores    q' = fl(q * fl(scale * log2 e)); a 16-lane team forms q' . k_j as four fmaf per lane and a four-level tree over the lanes.  Any summation
            order of hd products is within (hd - 1) U of sum |q'_d k_jd|, the rounding of q' adds U: (hd + 1) U A absolute on every score (the
            rounding of the constant is a common factor 1 + e, |e| <= U, of ALL scores and is counted with the arguments below).
  weights   The weight key j ends up with is fl(exp2(fl(s_j - m_t))) times the rescale factor fl(exp2(fl(m_old - m_new))) of every LATER tile of its
            team (one per tile, never one per key) times at most two merge weights (four teams of a wave, merged pairwise).  The arguments telescope to
            s_j - m, so the subtraction roundings and the common factor e together stay below 2 U x; every exp2 is v_exp_f32, 1 ulp = 2 U.  With R
            rescales that is a relative error of 2 U x + 2 U (R + 3) on p_j, on top of the score error entering as exp(ds_j - ds_max) <= 2 (hd + 1) U A.
            R <= ceil(ceil(Nk / 4) / 8) <= Nk / 32 + 1 where the keys are split over four teams (Nk > 8), R <= 4 on the short path (tiles of 2).
  ratio     o = sum_j p_j v_jc / sum_j p_j: a relative perturbation d of the weights moves the ratio by at most 2 d sum p |v| / sum p.
  sums      numerator and denominator each add at most Nk products one rounding apiece, take R rescale multiplications and two merges of two
            roundings: (Nk + R + 4) U of sum p |v| and of sum p; the final division adds U.

  |got - o| <= [2 ((hd + 1) U A + 2 U x + 2 U (R + 3)) + (2 (Nk + R + 4) + 1) U] sum p |v| / sum p
            <= [2 ((hd + 3) U A + 4 U (1 + x)) + (3 Nk + 32) U] sum p |v| / sum p                      (6 R <= Nk + 19 on both paths)

which is the form `bound` returns: the bracket's first part is the one stated with the kernel's contract, the last term has 3 Nk + 32 where a
two-pass softmax with one running sum would have Nk + 4, because of the per-tile rescales and the rigorous count of BOTH sums.  An indexing or tiling
mistake is an O(1) error, five orders of magnitude above this."""
import torch

U = 2.0 ** -24
TINY = 1e-300


def gather(flat, off, G0, G1, N, W, s0, s1, ld):
    """The cells the C ABI addresses, [G0, G1, N, W], from a flat buffer."""
    g0, g1 = torch.arange(G0).view(G0, 1, 1, 1), torch.arange(G1).view(1, G1, 1, 1)
    i, c = torch.arange(N).view(1, 1, N, 1), torch.arange(W).view(1, 1, 1, W)
    return flat[off + g0 * s0 + g1 * s1 + i * ld + c]


def cells(off, G0, G1, N, W, s0, s1, ld):
    g0, g1 = torch.arange(G0).view(G0, 1, 1, 1), torch.arange(G1).view(1, G1, 1, 1)
    i, c = torch.arange(N).view(1, 1, N, 1), torch.arange(W).view(1, 1, 1, W)
    return (off + g0 * s0 + g1 * s1 + i * ld + c).reshape(-1)


def attention64(q, k, v, H, scale=None):
    """q [G0, G1, Nq, H * hd], k, v [G0, G1, Nk, H * hd] (any float dtype) -> (o, bound), both fp64 [G0, G1, Nq, H * hd]."""
    G0, G1, Nq, W = q.shape
    Nk, hd = k.shape[2], W // H
    scale = hd ** -0.5 if scale is None else scale
    heads = lambda t: t.double().view(G0, G1, t.shape[2], H, hd).transpose(2, 3)            # [G0, G1, H, N, hd]
    q64, k64, v64 = heads(q), heads(k), heads(v)
    s = scale * (q64 @ k64.transpose(-1, -2))                                                  # [G0, G1, H, Nq, Nk]
    A = (abs(scale) * (q64.abs() @ k64.abs().transpose(-1, -2))).amax(-1, keepdim=True)
    m = s.amax(-1, keepdim=True)
    x = (s - m).abs().amax(-1, keepdim=True)
    p = (s - m).exp()
    den = p.sum(-1, keepdim=True)
    o = (p @ v64) / den
    mag = (p @ v64.abs()) / den
    bound = (2 * ((hd + 3) * U * A + 4 * U * (1 + x)) + (3 * Nk + 32) * U) * mag
    back = lambda t: t.transpose(2, 3).reshape(G0, G1, Nq, W)
    return back(o), back(bound)


def attention_strided64(qf, kf, vf, offs, G0, G1, Nq, Nk, H, hd, lds, strides, scale=None):
    """The C ABI's addressing restated: qf, kf, vf flat buffers, offs = (q, k, v) element offsets, lds = (ldq, ldk, ldv), strides = ((sq0, sq1), (sk0, sk1),
    (sv0, sv1)) -> (o, bound) dense [G0, G1, Nq, H * hd]."""
    W = H * hd
    q = gather(qf, offs[0], G0, G1, Nq, W, strides[0][0], strides[0][1], lds[0])
    k = gather(kf, offs[1], G0, G1, Nk, W, strides[1][0], strides[1][1], lds[1])
    v = gather(vf, offs[2], G0, G1, Nk, W, strides[2][0], strides[2][1], lds[2])
    return attention64(q, k, v, H, scale)
