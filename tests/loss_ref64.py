"""fp64 restatements of the sparse loss kernels (csrc/losses.hip: gd_pair_rank in its four forms, gd_depth_l1, gd_depth_head_fwd / _bwd, gd_smooth_ap
variants 0 and 1, gd_smooth_ap_me, gd_depth_bwd_combine, gd_scale_and_transpose), the per-element error bounds tests/test_gpu_loss_paths.py holds the
kernels to, the seeded inputs that file and tests/test_loss_ref_host.py share, and deliberately WRONG restatements (the `mut` arguments) that the host
test uses to show that the bounds are not vacuous.  Plain torch, CPU, fp64, explicit formulas, no autograd.  A test helper, not a test module.

Every operation is restated on the operands the kernel reads (u = W1 f as given, sim as given), so no upstream rounding enters a bound.

The head, for z [..., 128]:   mu = mean z, d = z - mu, var = mean d^2, rstd = (var + 1e-5)^-1/2, yh = d rstd, y = yh ln_w + ln_b,
  Phi = (1 + erf(y / sqrt 2)) / 2 (exact erf),  a = y Phi,  dg = Phi + y phi(y),  o = <a, w2> + b2,  s = tanh o
backward for dL = dLoss / ds:   dof = dL (1 - s^2),  dy = dof w2 dg,  dyh = dy ln_w,  m1 = mean dyh,  m2 = mean(dyh yh),
  dz = rstd (dyh - m1 - yh m2);   parameter gradients  b1: dz | ln_w: dy yh | ln_b: dy | w2: dof a | b2: dof   (the [513] layout of head_grad).

How a bound is formed.  A value travels as V(v, e): v the fp64 reference, e >= |kernel's fp32 value - v| to first order.  Each fp32 operation of the
kernel is one function below that forms v exactly and e from the operands' |v| and e — first-order propagation with the |.| sums evaluated in fp64
beside the reference — plus the operation's own rounding.  Constants, as in tests/cv_ref64.py:
  U = 2^-24: one fp32 rounding (add, sub, mul: U |result|; a fused multiply-add rounds once: charging both is valid);
  __expf, __logf, v_rcp, v_rsq, expf, log1pf, tanhf, sqrtf, a division: 2 U each; __expf(x) scales x by log2 e first: (2 + |x|) U relative;
  __logf is a scaled v_log: absolute 2 U max(|log x|, 1);
  a reduction of n terms whose order nothing fixes (LDS and global atomics: du, the head gradients, the loss and count sums, the smooth-AP row
  sums): n U sum|terms|;  a 128-channel sum inside one head evaluation has a fixed shape in every form — 2, 8 or 16 channels chained in a lane,
  then 6, 4 or 3 shuffle steps — so a channel passes at most CH = 20 additions there: CH U sum|terms| (the depth charge of cv_ref64's NT and NS);
  SECOND = 2: every output's first-order bound is multiplied once for the dropped higher-order terms.
One constant comes from the kernels' documented method: gelu_parts is the Abramowitz-Stegun 7.1.26 erfc, |eps| <= 1.5e-7, so Phi carries
PHI_ABS = 7.5e-8 absolute, in a and in GELU' alike; its evaluation (v_rcp, a five-term Horner chain, one __expf, the products) is charged from its own
operations (_phi).  The 8- and 16-lane forms take tanh as 1 - 2 rcp(1 + e^2o): (1 - s^2)(|o| + 1) U from the exponential, 3 U (1 - s) from the sum and
the reciprocal, U |s| from the subtraction; tanhf of the wave-per-pair form is 2 U |s|: e_tanh = (1 - s^2)(|o| + 1) U + 3 U (1 - s) + 3 U |s| covers
both, and 1 - s^2 = 1 - fl(s s) then carries 2 |s| e_s + U s^2 + U (1 - s^2) ABSOLUTE (a saturated head has no relative bound).
Errors that are ONE fp32 number per head evaluation are carried as such, through exact partial derivatives, instead of as 128 separate |.| terms
(class Head): the errors of mu and rstd on their way to o, and the error of dof = dL (1 - s^2), which multiplies every channel of dz and of the
parameter gradients in all four forms (the lane forms compute rstd dof (q ln_w - P1 - yh P2), q = w2 dg, the wave form distributes dof first: the
products are charged for the longer order, 4 U on dz).
No constant is tuned against a kernel's output.  Structural zeros (du rows at or beyond counts, dsim rows and columns at or beyond counts,
head_grad_sets[:, 513:], a smooth-AP gradient whose two sigmoids are both outside the exponent clamp) have bound 0.
gd_scale_and_transpose is one fp32 product: the test requires torch.equal with the fp32 product.

Comparisons (a depth mask |d_j - d_i| > thr, a 3-D distance against a threshold, the exponent clamp at +-50, the sign of an L1 residual) are
decided in fp64 from the fp32 inputs; the input builders keep every one of them away from its threshold by more than fp32 arithmetic can move it,
and `ambiguous_*` count the ones that are not: tests/test_loss_ref_host.py asserts the counts are zero, nothing is ever excluded from a comparison."""
import math

import torch

from cv_ref64 import SECOND, U

F64 = torch.float64
PHI_ABS = 7.5e-8
LN_EPS = 1e-5
CH = 20                        # additions a channel passes in a 128-channel sum: see the module docstring
HG = 516                       # floats per head-gradient row: b1 | ln_w | ln_b | w2 | b2 | 3 x zero
AS_P = 0.3275911
AS_C = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
SQRT1_2 = 0.70710678118654752
INV_SQRT_2PI = 0.39894228040143268


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------ values with first-order bounds
class V:
    """v: fp64 reference; e >= |fp32 value - v| to first order (before SECOND)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v if torch.is_tensor(v) else torch.tensor(float(v), dtype=F64)
        self.e = torch.zeros_like(self.v) if e is None else e

    def __getitem__(self, k):
        return V(self.v[k], self.e[k])


def _v(x):
    return x if isinstance(x, V) else V(x.double() if torch.is_tensor(x) else x)


def add(a, b, k=1):
    a, b = _v(a), _v(b)
    v = a.v + b.v
    return V(v, a.e + b.e + k * U * v.abs())


def sub(a, b, k=1):
    a, b = _v(a), _v(b)
    v = a.v - b.v
    return V(v, a.e + b.e + k * U * v.abs())


def mul(a, b, k=1):
    a, b = _v(a), _v(b)
    v = a.v * b.v
    return V(v, a.v.abs() * b.e + b.v.abs() * a.e + k * U * v.abs())


def div(a, b, k=2):
    a, b = _v(a), _v(b)
    v = a.v / b.v
    return V(v, a.e / b.v.abs() + v.abs() * b.e / b.v.abs() + k * U * v.abs())


def scale(a, c):
    """times a power of two, a sign or a 0/1 mask: exact."""
    c = c if torch.is_tensor(c) else torch.tensor(float(c), dtype=F64)
    return V(a.v * c, a.e * c.abs())


def fn(a, f, absdf, k):
    """v = f(a), e = |f'(a)| e_a + k U |v|  (k may be a tensor)."""
    v = f(a.v)
    return V(v, absdf(a.v) * a.e + k * U * v.abs())


def total(a, dim, n=None, keepdim=False):
    """sum over dim in any order: n U sum|terms| (n: the number of terms, default the extent)."""
    if n is None:
        n = a.v.shape[dim] if isinstance(dim, int) else math.prod(a.v.shape[d] for d in dim)
    return V(a.v.sum(dim, keepdim=keepdim), a.e.sum(dim, keepdim=keepdim) + n * U * a.v.abs().sum(dim, keepdim=keepdim))


def bound(a):
    return SECOND * a.e


# ------------------------------------------------------------------------------------------------ the head
def _phi(y, gelu="erf"):
    """-> (Phi, ex = exp(-y^2 / 2)) as gelu_parts forms them.  Phi's value is the exact one; its bound: phi(y) e_y, PHI_ABS, and the evaluation:
    t = rcp(1 + p |y| / sqrt 2): 5 U relative;  the Horner chain h_k = c_k + t h_k+1, poly = t h_1: U (|t h_k+1| + |h_k|) t^(k-1) per step, and
    |poly'(t)| e_t;  ex: (2 + 1.5 y^2) U relative (y y, the half, the log2 e scaling, v_exp);  tail = poly ex / 2: 2 U;  1 - tail: U."""
    ex = fn(scale(mul(y, y), -0.5), torch.exp, torch.exp, 2 + 0.5 * y.v * y.v)
    ay = y.v.abs()
    t = 1.0 / (1.0 + AS_P * SQRT1_2 * ay)
    h = torch.full_like(t, AS_C[4])
    dh = torch.zeros_like(t)                                   # d h / d t
    rnd = torch.zeros_like(t)
    for c in AS_C[3::-1]:
        dh = h + t * dh
        hn = c + t * h
        rnd = rnd * t + U * ((t * h).abs() + hn.abs())
        h = hn
    dpoly = (h + t * dh).abs()
    rnd = rnd * t + U * (t * h).abs()
    tail = 0.5 * torch.erfc(ay * SQRT1_2)
    phi = torch.exp(-0.5 * y.v * y.v) * INV_SQRT_2PI
    e0 = 0.5 * ex.v * (dpoly * 5 * U * t + rnd) + tail * ((2 + 1.5 * y.v * y.v) * U + 2 * U) + PHI_ABS
    Phi = 0.5 * (1.0 + torch.erf(y.v * SQRT1_2))
    if gelu == "tanh":                                          # mutant: the tanh-form GELU, a = y Phi_t(y)
        Phi = 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (y.v + 0.044715 * y.v ** 3)))
    return V(Phi, phi * y.e + e0 + U * Phi), ex


def _act(yh, hp, gelu):
    """yh (V) -> (a = GELU(y), dg = GELU'(y)), y = yh ln_w + ln_b."""
    y = add(mul(yh, hp["ln_w"].double()), hp["ln_b"].double())
    Phi, ex = _phi(y, gelu)
    return mul(y, Phi), add(Phi, mul(mul(y, ex), INV_SQRT_2PI, 2))


class Head:
    """The forward of one batch of head evaluations z [..., 128] (V) and what its backward needs.

    The errors of mu and of rstd are two SCALARS per evaluation, common to its 128 channels: where they reach another scalar, o, they do so through
    the exact partial derivatives  d o / d mu = -rstd sum_k w2 dg ln_w  and  d o / d log rstd = sum_k w2 dg ln_w yh  (signed sums, which mostly
    cancel), not through 128 separate |.| terms; only each channel's own roundings are summed in absolute value.  To first order var does not see
    the error of mu at all (d var / d mu = -2 mean d = 0).  The channel-wise quantities of the backward (yh, a, dg) carry all three parts."""

    def __init__(self, z, hp, eps=LN_EPS, gelu="erf"):
        self.hp = hp
        lw, w2 = hp["ln_w"].double(), hp["w2"].double()
        mu = scale(total(z, -1, CH, keepdim=True), 1.0 / 128)
        dv = z.v - mu.v
        d = V(dv, z.e + U * dv.abs())                            # without e_mu
        var = scale(total(mul(d, d), -1, CH, keepdim=True), 1.0 / 128)
        self.rstd = fn(add(var, eps), torch.rsqrt, lambda x: 0.5 * x ** -1.5, 2)
        yh_own = mul(d, V(self.rstd.v))                          # each channel's own roundings
        rr = self.rstd.e / self.rstd.v
        self.yh = V(yh_own.v, yh_own.e + self.rstd.v * mu.e + yh_own.v.abs() * rr)
        a_own, dg_own = _act(yh_own, hp, gelu)
        o_own = total(mul(a_own, w2), -1, CH)
        t = w2 * dg_own.v * lw
        common = t.sum(-1).abs() * self.rstd.v[..., 0] * mu.e[..., 0] + (t * yh_own.v).sum(-1).abs() * rr[..., 0]
        self.o = add(V(o_own.v, o_own.e + common), hp["b2"].double().reshape(()))
        self.a, self.dg = _act(self.yh, hp, gelu)
        s = torch.tanh(self.o.v)
        oms = 1.0 - s * s
        self.s = V(s, oms * self.o.e + oms * (self.o.v.abs() + 1) * U + 3 * U * (1 - s) + 3 * U * s.abs())
        self.oms = V(oms, 2 * s.abs() * self.s.e + U * s * s + U * oms)

    def back(self, dL):
        """dL [...] (V) -> dz [..., 128] and the per-evaluation parameter gradients {b1, ln_w, ln_b, w2 [..., 128], b2 [...]}.  dof = dL (1 - s^2) is
        one fp32 number that multiplies every channel in every form: its error is carried as the common factor it is, dz = dof G with
        G = rstd (q ln_w - P1 - yh P2), q = w2 dg, P1 = mean(q ln_w), P2 = mean(q ln_w yh); the products are charged for the longer of the two
        orders of evaluation (4 U on dz, 3 U on the parameter gradients)."""
        lw, w2 = self.hp["ln_w"].double(), self.hp["w2"].double()
        dof = mul(dL, self.oms)
        dofc = V(dof.v[..., None], dof.e[..., None])
        q = mul(self.dg, w2)
        ql = mul(q, lw)
        P1 = scale(total(ql, -1, CH, keepdim=True), 1.0 / 128)
        P2 = scale(total(mul(ql, self.yh), -1, CH, keepdim=True), 1.0 / 128)
        G = mul(sub(sub(ql, P1), mul(self.yh, P2)), self.rstd)
        dz = mul(dofc, G, 4)
        return dz, {"b1": dz, "ln_w": mul(dofc, mul(q, self.yh), 3), "ln_b": mul(dofc, q, 3), "w2": mul(dofc, self.a, 3), "b2": dof}


def _pack_hg(parts, swap_ln=False):
    """{b1, ln_w, ln_b, w2 [128], b2 []} (V) -> [516] (V) in the head_grad layout, the last three zero."""
    order = ["b1", "ln_b", "ln_w", "w2"] if swap_ln else ["b1", "ln_w", "ln_b", "w2"]
    z3 = torch.zeros(3, dtype=F64)
    return V(torch.cat([parts[k].v for k in order] + [parts["b2"].v.reshape(1), z3]),
             torch.cat([parts[k].e for k in order] + [parts["b2"].e.reshape(1), z3]))


def _zeros(*shape):
    return V(torch.zeros(shape, dtype=F64))


def _stack(vs):
    return V(torch.stack([t.v for t in vs]), torch.stack([t.e for t in vs]))


# ------------------------------------------------------------------------------------------------ gd_pair_rank
def rank_valid(depth, thr, ge=False):
    """depth [n] fp32 -> (valid [n, n] bool over ordered pairs (i, j), alpha = sign(d_j - d_i), dd)."""
    dd = depth.double()[None, :] - depth.double()[:, None]
    return (dd.abs() >= f32(thr)) if ge else (dd.abs() > f32(thr)), torch.sign(dd), dd


def rank_set(u, depth, thr, hp, g=1.0, eps=LN_EPS, gelu="erf", mask_ge=False, drop_mirror=False, drop_pair=None, mean_n2=False, swap_ln=False,
             want_pairs=False):
    """One keypoint set of gd_pair_rank: u [n, 128], depth [n] fp32 (the rows inside counts), g = gscale of the set.
    -> dict(loss V [], du V [n, 128], hg V [516], cnt int); want_pairs adds dz V [n, n, 128] (dLoss_sum / dz of pair (i, j), unscaled), valid, o."""
    n = u.shape[0]
    if n == 0:
        return dict(loss=_zeros(), du=_zeros(0, 128), hg=_zeros(HG), cnt=0)
    ud = u.double()
    delta = ud[None, :, :] - ud[:, None, :]                       # [i, j] = u_j - u_i, one fp32 subtraction (its negation is exact)
    H = Head(add(V(delta, U * delta.abs()), hp["b1"].double()), hp, eps, gelu)
    valid, alpha, _ = rank_valid(depth, thr, mask_ge)
    m = valid.double()
    if drop_pair is not None and max(drop_pair) < n:
        m[drop_pair] = 0.0
    cnt = int(valid.sum())
    em = fn(scale(H.s, -alpha), torch.exp, torch.exp, 2 + H.s.v.abs())
    one_em = add(em, 1.0)
    lg = torch.log(one_em.v)
    ell = V(lg, one_em.e / one_em.v + 2 * U * lg.abs().clamp_min(1.0))
    dL = scale(div(em, one_em, 3), -alpha)                        # -alpha / (1 + e^(alpha s)) = -alpha em rcp(1 + em)
    dz, parts = H.back(dL)
    partners = m.sum(1)                                           # valid partners of row i (the mask is symmetric)
    n_row = (2 * partners + 16)[:, None]                          # 2 terms per partner, the tile partials of the tiled form
    own = total(scale(dz, -m[:, :, None]), 1, n_row)              # pair (i, j): z = u_j - u_i + b1, d z / d u_i = -1
    mirror = total(scale(dz, m[:, :, None]), 0, n_row)            # pair (j, i) seen from its second keypoint: + dz[j, i]
    du = own if drop_mirror else add(own, mirror, 0)
    n_all = cnt + 16
    hg = _pack_hg({k: total(scale(p, m[:, :, None] if p.v.dim() == 3 else m), (0, 1), n_all) for k, p in parts.items()}, swap_ln)
    lsum = total(scale(ell, m), (0, 1), n_all)
    out = dict(cnt=cnt)
    if cnt == 0:
        out.update(loss=_zeros(), du=_zeros(n, 128), hg=_zeros(HG))
    else:
        den = float(n * n) if mean_n2 else float(cnt)
        sc = div(V(torch.tensor(f32(g), dtype=F64)), den)
        out.update(loss=div(lsum, den, 1), du=mul(du, sc), hg=mul(hg, sc))
    if want_pairs:
        out.update(dz=dz, valid=valid, o=H.o.v, sc=(f32(g) / cnt if cnt else 0.0))
    return out


def rank_case(inp, **mut):
    """gd_pair_rank on a RankInputs -> dict(loss V [S], du V [S, Nmax, 128] (rows at or beyond counts: 0 with bound 0), hg_sets V [S, 516],
    hg_sum V [516] = what head_grad gains (see head_grad_bound), cnt [S] int)."""
    S, Nmax = inp.u.shape[:2]
    du = _zeros(S, Nmax, 128)
    loss, hgs, cnt = [], [], []
    for s in range(S):
        n = inp.n(s)
        r = rank_set(inp.u[s, :n], inp.depth[s, :n], inp.thr, inp.hp, 1.0 if inp.gscale is None else float(inp.gscale[s]), **mut)
        du.v[s, :n], du.e[s, :n] = r["du"].v, r["du"].e
        loss.append(r["loss"])
        hgs.append(r["hg"])
        cnt.append(r["cnt"])
    hgs = _stack(hgs)
    return dict(loss=_stack(loss), du=du, hg_sets=hgs, hg_sum=total(hgs, 0, S + 1), cnt=cnt)


def head_grad_bound(hg_sum, prefill, n_adds):
    """head_grad arrives holding `prefill` and gains the sum in n_adds additions (atomic, any order): the sum's own bound and n_adds roundings of
    the prefill (the running sum's share is in hg_sum's reduction charge)."""
    return bound(hg_sum) + SECOND * n_adds * U * abs(prefill)


# ------------------------------------------------------------------------------------------------ gd_depth_l1, gd_depth_head
def l1_case(inp, **mut):
    """gd_depth_l1 on an L1Inputs -> dict(loss V [P], du V [P, 2, Nmax, 128], hg_sets V [P, 516], hg_sum V [516], resid [sum n] = s - t with the
    bound on it, for ambiguous_l1)."""
    P, _, Nmax, _ = inp.u.shape
    du = _zeros(P, 2, Nmax, 128)
    loss, hgs, resid = [], [], []
    for p in range(P):
        n = inp.n(p)
        if n == 0:
            loss.append(_zeros())
            hgs.append(_zeros(HG))
            continue
        u1, u2 = inp.u[p, 0, :n].double(), inp.u[p, 1, :n].double()
        dlt = u1 - u2
        H = Head(add(V(dlt, U * dlt.abs()), inp.hp["b1"].double()), inp.hp, **mut)
        dd = inp.d1[p, :n].double() - inp.d2[p, :n].double()
        t = fn(V(dd, U * dd.abs()), torch.tanh, lambda x: 1 - torch.tanh(x) ** 2, 2)
        diff = sub(H.s, t)
        resid.append(torch.stack([diff.v, diff.e]))
        w = div(V(torch.tensor(1.0 if inp.gscale is None else f32(float(inp.gscale[p])), dtype=F64)), float(n))
        dz, parts = H.back(mul(V(torch.sign(diff.v)), w, 0))
        du.v[p, 0, :n], du.e[p, 0, :n], du.v[p, 1, :n], du.e[p, 1, :n] = dz.v, dz.e, -dz.v, dz.e
        hgs.append(_pack_hg({k: total(q, 0, n + 8) for k, q in parts.items()}))
        loss.append(total(div(V(diff.v.abs(), diff.e), float(n)), 0, n + 8))
    hgs = _stack(hgs)
    return dict(loss=_stack(loss), du=du, hg_sets=hgs, hg_sum=total(hgs, 0, P + 1), resid=torch.cat(resid, 1))


def head_rows(u, hp, dout=None, **mut):
    """gd_depth_head_fwd / _bwd on rows u [M, 128] -> (out V [M], du V [M, 128] | None, hg V [516] | None)."""
    H = Head(add(V(u.double()), hp["b1"].double()), hp, **mut)
    if dout is None:
        return H.s, None, None
    dz, parts = H.back(V(dout.double()))
    return H.s, dz, _pack_hg({k: total(q, 0, u.shape[0] + 8) for k, q in parts.items()})


# ------------------------------------------------------------------------------------------------ smooth-AP
def inv_temp(temp):
    return float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(temp, dtype=torch.float32))


def sig_t(x, inv, zero_outside=True):
    """sig_t of the kernel: e = -x inv, y = 1 / (1 + exp(clamp(e, +-50))), dsig = y (1 - y) inv inside the clamp and exactly 0 outside.
    -> (y, dsig, e.v)"""
    e = mul(x, -inv)
    inside = ((e.v >= -50.0) & (e.v <= 50.0)).double()
    ec = V(e.v.clamp(-50.0, 50.0), e.e * inside)
    y = div(1.0, add(fn(ec, torch.exp, torch.exp, 2), 1.0))
    ds = mul(mul(y, sub(1.0, y)), inv)
    return y, (scale(ds, inside) if zero_outside else ds), e.v


def _dist(p1, p2):
    d = p1.double()[:, None, :] - p2.double()[None, :, :]
    return d.pow(2).sum(-1).sqrt()


def _ap(r, A):
    den = add(r, A)
    ap = div(r, den)
    den2 = mul(den, den)
    return ap, scale(div(r, den2), -1.0), div(A, den2)             # ap, d ap / d A, d ap / d r


def ap_pair(sim, p1, p2, variant, thr, temp, diag_neg=False, swap_variant=False, zero_outside=True):
    """One pair of gd_smooth_ap inside its counts: sim [n, n] fp32 -> (rows V [n] = row_ws, dsim V [n, n])."""
    n = sim.shape[0]
    inv = inv_temp(temp)
    s = sim.double()
    eye = torch.eye(n, dtype=torch.bool)
    neg = (_dist(p1, p2) > f32(thr)) & (torch.ones_like(eye) if diag_neg else ~eye)
    m = neg.double()
    pos = s.diagonal()
    x1, x2 = s - 1.0, s - pos[:, None]
    y1, d1, _ = sig_t(V(x1, U * x1.abs()), inv, zero_outside)
    y2, d2, _ = sig_t(V(x2, U * x2.abs()), inv, zero_outside)
    nn = m.sum(1) + 8
    A1, A2, D2 = total(scale(y1, m), 1, nn), total(scale(y2, m), 1, nn), total(scale(d2, m), 1, nn)
    xp = 1.0 - pos
    ya, da, _ = sig_t(V(xp, U * xp.abs()), inv, zero_outside)       # sig(1 - pos): d / d pos = -da
    yb, db, _ = sig_t(V(-xp, U * xp.abs()), inv, zero_outside)      # sig(pos - 1): d / d pos = +db
    first_is_a = (variant == 0) != swap_variant
    r1, dr1 = (add(ya, 1.0), scale(da, -1.0)) if first_is_a else (add(yb, 1.0), db)
    r2, dr2 = add(ya, 1.0), scale(da, -1.0)
    ap1, dA1, dR1 = _ap(r1, A1)
    ap2, dA2, dR2 = _ap(r2, A2)
    w = div(-0.5, float(n), 1)
    rows = div(sub(1.0, scale(add(ap1, ap2), 0.5)), float(n))
    off = mul(add(mul(dA1[:, None], d1), mul(dA2[:, None], d2)), w)
    dg = mul(sub(add(mul(dR1, dr1), mul(dR2, dr2)), mul(dA2, D2)), w)
    off = scale(off, m * (~eye).double())
    return rows, V(off.v + torch.diag(dg.v), off.e + torch.diag(dg.e))


def ap_case(inp, variant, **mut):
    """gd_smooth_ap -> dict(loss V [P], rows V [P, Nmax], dsim V [P, Nmax, Nmax]); everything at or beyond counts is 0 with bound 0."""
    P, Nmax = inp.sim.shape[:2]
    rows, dsim = _zeros(P, Nmax), _zeros(P, Nmax, Nmax)
    for p in range(P):
        n = inp.n(p)
        r, d = ap_pair(inp.sim[p, :n, :n], inp.p1[p, :n], inp.p2[p, :n], variant, inp.thr_neg, inp.temp, **mut)
        rows.v[p, :n], rows.e[p, :n], dsim.v[p, :n, :n], dsim.e[p, :n, :n] = r.v, r.e, d.v, d.e
    return dict(loss=total(rows, 1, Nmax), rows=rows, dsim=dsim)


def me_pair(sim, p1, p2, thr_pos, thr_neg, temp, per_rows=False):
    """One pair of gd_smooth_ap_me inside its counts -> (loss V [], row_ws V [n, 2] = {sum over the row's positives of 1 - ap, their number},
    dsim V [n, n])."""
    n = sim.shape[0]
    inv = inv_temp(temp)
    s = sim.double()
    dist = _dist(p1, p2)
    m = (dist > f32(thr_neg)).double()
    posm = dist < f32(thr_pos)
    y1, d1, _ = sig_t(V(s - 1.0, U * (s - 1.0).abs()), inv)
    nn = m.sum(1) + 8
    A1 = total(scale(y1, m), 1, nn)
    lrow, dsim = _zeros(n), _zeros(n, n)
    npos = posm.sum(1)
    for k in range(int(npos.max()) if n else 0):                   # the k-th positive of every row that has one
        has = npos > k
        jp = torch.where(has, (posm.long().cumsum(1) == k + 1).long().argmax(1), torch.zeros(n, dtype=torch.long))
        hm = has.double()
        pos = s.gather(1, jp[:, None])[:, 0]
        x2 = s - pos[:, None]
        y2, d2, _ = sig_t(V(x2, U * x2.abs()), inv)
        A2, D2 = total(scale(y2, m), 1, nn), total(scale(d2, m), 1, nn)
        xp = pos - 1.0
        ya, da, _ = sig_t(V(xp, U * xp.abs()), inv)                # r1 = sig(pos - 1) + 1
        yb, db, _ = sig_t(V(-xp, U * xp.abs()), inv)               # r2 = sig(1 - pos) + 1
        ap1, dA1, dR1 = _ap(add(ya, 1.0), A1)
        ap2, dA2, dR2 = _ap(add(yb, 1.0), A2)
        lrow = add(lrow, scale(sub(1.0, scale(add(ap1, ap2), 0.5)), hm))
        off = scale(add(mul(dA1[:, None], d1), mul(dA2[:, None], d2)), -0.5 * m * hm[:, None])
        dgp = scale(sub(sub(mul(dR1, da), mul(dR2, db)), mul(dA2, D2)), -0.5 * hm)
        onehot = torch.zeros(n, n, dtype=F64).scatter_(1, jp[:, None], 1.0)
        dsim = add(dsim, add(off, V(onehot * dgp.v[:, None], onehot * dgp.e[:, None])))
    M = float(npos.sum())
    row_ws = V(torch.stack([lrow.v, npos.double()], 1), torch.stack([lrow.e, torch.zeros(n, dtype=F64)], 1))
    if M == 0:
        return _zeros(), row_ws, _zeros(n, n)
    den = float((npos > 0).sum()) if per_rows else M
    invM = div(1.0, den)
    return mul(total(lrow, 0, n + 8), invM), row_ws, mul(dsim, invM)


def me_case(inp, **mut):
    P, Nmax = inp.sim.shape[:2]
    rows, dsim, loss = _zeros(P, Nmax, 2), _zeros(P, Nmax, Nmax), []
    for p in range(P):
        n = inp.n(p)
        ls, r, d = me_pair(inp.sim[p, :n, :n], inp.p1[p, :n], inp.p2[p, :n], inp.thr_pos, inp.thr_neg, inp.temp, **mut)
        rows.v[p, :n], rows.e[p, :n], dsim.v[p, :n, :n], dsim.e[p, :n, :n] = r.v, r.e, d.v, d.e
        loss.append(ls)
    return dict(loss=_stack(loss), rows=rows, dsim=dsim)


# ------------------------------------------------------------------------------------------------ gd_depth_bwd_combine
def combine(du_r, du_l, hg_r, hg_l, g_l1, g_intra, view_major):
    """du_r, du_l [P, 2, N, 128], hg_r [2P, 516], hg_l [P, 516], g_l1, g_intra [P] fp32 -> (du_out V [2 P N, 128] rows in pair-major or view-major
    order, hg_out V [516])."""
    P, _, N, _ = du_r.shape
    gi = scale(V(g_intra.double()), 0.5)
    gl = V(g_l1.double())
    du = add(mul(du_r, gi.v[:, None, None, None]), mul(du_l, gl.v[:, None, None, None]))
    if view_major:
        du = V(du.v.transpose(0, 1).contiguous(), du.e.transpose(0, 1).contiguous())
    hr = hg_r.double().view(P, 2, HG)
    terms = add(mul(gi.v[:, None], add(hr[:, 0], hr[:, 1])), mul(gl.v[:, None], hg_l))
    return V(du.v.reshape(2 * P * N, 128), du.e.reshape(2 * P * N, 128)), total(terms, 0, P)


# ------------------------------------------------------------------------------------------------ the shared inputs
def head_params(seed, w2_scale):
    """ln_w, ln_b not trivial, b2 != 0; w2_scale sets the spread of the pre-tanh value."""
    g = torch.Generator().manual_seed(seed)
    return {"b1": 0.1 * torch.randn(128, generator=g), "ln_w": 1.0 + 0.3 * torch.randn(128, generator=g), "ln_b": 0.2 * torch.randn(128, generator=g),
            "w2": w2_scale * torch.randn(128, generator=g), "b2": torch.tensor([0.15])}


def ambiguous_pairs(depth, counts, thr, margin=1e-5):
    """ordered pairs inside counts with | |d_j - d_i| - thr | < margin, |.| == thr exactly excepted when the subtraction is exact (multiples of 1/8)."""
    bad = 0
    for s in range(depth.shape[0]):
        n = depth.shape[1] if counts is None else int(counts[s])
        dd = (depth[s, :n].double()[None] - depth[s, :n].double()[:, None]).abs()
        exact = (depth[s, :n] * 8 == (depth[s, :n] * 8).round()).all()
        near = (dd - f32(thr)).abs() < margin
        bad += int((near & (dd != f32(thr))).sum()) if exact else int(near.sum())
    return bad


class _Counted:
    def n(self, s):
        return self.Nmax if self.counts is None else int(self.counts[s])


class RankInputs(_Counted):
    def __init__(self, name, u, depth, counts, gscale, thr, hp):
        self.name, self.u, self.depth, self.counts, self.gscale, self.thr, self.hp = name, u, depth, counts, gscale, thr, hp
        self.S, self.Nmax = u.shape[:2]


GSCALES = [1.0, 0.0, -0.5, 2.0, 0.75, 1.25]                       # per set: a zero and a negative one among them
RANK_THR = 0.05
# name -> (Nmax, counts, feature scale, per-set gscale or None)
RANK_CASES = {
    "ragged_1": (40, [40, 34, 18, 17, 1, 0], 1.0, GSCALES),                # 18: valid pairs and padding slots in one wave; 17: row 16 alone
    "ragged_0.05": (40, [40, 34, 18, 17, 1, 0], 0.05, None),
    "seams_full": (70, None, 1.0, None),                                   # 5 x 3 tiles of 16 x 32, neither extent a multiple
    "seams_counts": (70, [70, 65, 64, 33, 32, 31], 0.05, GSCALES),
    "exact_mask": (40, [40, 34, 18, 17, 1, 0], 1.0, GSCALES),
}
# Two heads per case, because two conditions on the inputs exclude each other under these bounds (tests/test_loss_ref_host.py asserts both):
#   "active":     every valid ordered pair moves some du element by more than 4 x its bound (a dropped pair cannot hide): |o| stays below 3;
#   "saturating": the pre-tanh value spans more than [-4, 4] over the valid pairs: the saturated branch of tanh and of 1 - s^2 is exercised, where a
#                 pair's gradient (1 - s^2 ~ 1e-3) is below the bound of the 2 (n - 1)-term row sum it joins.
# w2 scale by (head, feature scale): LayerNorm removes the feature scale only where the differences dominate b1.
HEADS = {("active", 1.0): 0.08, ("active", 0.05): 0.12, ("saturating", 1.0): 0.3, ("saturating", 0.05): 0.6}
HEAD_NAMES = ("active", "saturating")
SEAM_PAIR = (15, 32)                                              # last row of tile row 0, first column of tile column 1


def rank_inputs(name, head="active"):
    Nmax, counts, fscale, gs = RANK_CASES[name]
    S = 6
    g = torch.Generator().manual_seed(1000 + sorted(RANK_CASES).index(name))
    u = fscale * torch.randn(S, Nmax, 128, generator=g)
    cts = None if counts is None else torch.tensor(counts, dtype=torch.int32)
    if name == "exact_mask":
        # multiples of 1/8 and thr = 0.25: |d_j - d_i| == thr (excluded: the mask is strict) and equal depths both occur, every fp32 subtraction exact
        thr = 0.25
        depth = torch.randint(0, 12, (S, Nmax), generator=g).float() / 8
        depth[:, 0], depth[:, 1], depth[:, 2], depth[:, 3] = 0.5, 0.75, 0.5, 1.5
        depth[:, 16], depth[:, 17], depth[:, 32], depth[:, 33] = 0.0, 1.0, 0.125, 1.25      # counts 18 and 34: a valid pair beside two padding slots
        u[:, 3] = u[:, 0]                                          # identical feature rows, different depths
    else:
        thr = RANK_THR
        while True:
            depth = torch.rand(S, Nmax, generator=g) * 3
            depth[:, SEAM_PAIR[0]], depth[:, SEAM_PAIR[1]] = 0.4, 2.2      # the seam pair is a valid one wherever both are inside counts
            if ambiguous_pairs(depth, None, thr) == 0:
                break
    return RankInputs(name, u, depth, cts, None if gs is None else torch.tensor(gs), thr, head_params(7, HEADS[(head, fscale)]))


class L1Inputs(_Counted):
    def __init__(self, u, d1, d2, counts, gscale, hp):
        self.u, self.d1, self.d2, self.counts, self.gscale, self.hp = u, d1, d2, counts, gscale, hp
        self.Nmax = u.shape[2]


def l1_inputs(fscale=1.0, with_gscale=True):
    """P = 4, Nmax = 21 (a 16-keypoint block and 5 more), counts [21, 16, 5, 0]."""
    g = torch.Generator().manual_seed(2000 + int(fscale * 100))
    P, Nmax = 4, 21
    u = fscale * torch.randn(P, 2, Nmax, 128, generator=g)
    d1, d2 = torch.rand(P, Nmax, generator=g) * 3, torch.rand(P, Nmax, generator=g) * 3
    return L1Inputs(u, d1, d2, torch.tensor([21, 16, 5, 0], dtype=torch.int32), torch.tensor(GSCALES[:4]) if with_gscale else None, head_params(7, 0.2))


def ambiguous_l1(resid):
    """L1 residuals whose sign the bound cannot tell: |s - t| <= 4 x bound."""
    return int((resid[0].abs() <= 4 * SECOND * resid[1]).sum())


HEAD_M = [1, 31, 32, 33, 70]                                      # 32 rows per block of gd_depth_head_*


def head_inputs(M, fscale=1.0):
    g = torch.Generator().manual_seed(3000 + M)
    return fscale * torch.randn(M, 128, generator=g), torch.randn(M, generator=g), head_params(7, 0.2)


class ApInputs(_Counted):
    def __init__(self, sim, p1, p2, counts, thr_pos, thr_neg, temp):
        self.sim, self.p1, self.p2, self.counts, self.thr_pos, self.thr_neg, self.temp = sim, p1, p2, counts, thr_pos, thr_neg, temp
        self.Nmax = sim.shape[1]


AP_SHAPES = {"stride": (4, 264, [264, 257, 256, 1]), "small": (2, 24, None)}      # 264: past the 256-thread stride of a row


def _sim(g, P, N, temp):
    """sim built directly: positives (the diagonal) in [0.7, 1]; every other entry placed against its row's positive or against 1 so that
    (s - pos) / temp and (s - 1) / temp cover |.| < 5, both sides beyond +-50, and +-50 (1 -+ 1e-3), just inside and just outside the clamp."""
    pos = 0.7 + 0.3 * torch.rand(P, N, generator=g, dtype=F64)
    kind = torch.randint(0, 8, (P, N, N), generator=g)
    t = torch.rand(P, N, N, generator=g, dtype=F64) * 10 - 5
    sgn = torch.where(torch.rand(P, N, N, generator=g) < 0.5, -1.0, 1.0).double()
    edge = sgn * 50 * (1 + torch.where(torch.rand(P, N, N, generator=g) < 0.5, -1e-3, 1e-3).double())
    far = sgn * (60 + 30 * torch.rand(P, N, N, generator=g, dtype=F64))
    base = torch.where(kind % 2 == 0, pos[:, :, None].expand(P, N, N), torch.ones(P, N, N, dtype=F64))
    off = torch.where(kind < 4, t, torch.where(kind < 6, far, edge))
    sim = base + temp * off
    idx = torch.arange(N)
    sim[:, idx, idx] = pos
    return sim.float()


def _near_clamp(sim, posm, temp, rel=2e-4):
    """[N, N] bool: off-positive entries of one pair's sim with a sigmoid exponent within `rel` of the clamp at +-50."""
    s, inv = sim.double(), inv_temp(temp)

    def near(x):
        return ((x * inv).abs() - 50.0).abs() < 50.0 * rel

    bad = near(s - 1.0)
    for i, jp in torch.nonzero(posm).tolist():
        bad[i] |= near(s[i] - s[i, jp])
    return bad & ~posm


def ap_inputs(shape, me=False):
    """sim, 3-D points and counts of a smooth-AP case (me: for gd_smooth_ap_me, positives by distance).  Points are redrawn until no distance is
    within a relative 1e-4 of a threshold; a sim entry whose exponent falls within 2e-4 of the clamp by chance is moved far outside it."""
    P, N, counts = AP_SHAPES[shape]
    g = torch.Generator().manual_seed(4000 + N + (1 if me else 0))
    temp, thr_neg, thr_pos = 0.01, 0.1, 5e-3
    sim = _sim(g, P, N, temp)
    empty = P - 1 if counts is None else 1                         # ME: the pair with no positive at all
    while True:
        p1 = torch.rand(P, N, 3, generator=g)
        p2 = p1 + 1e-3 * torch.randn(P, N, 3, generator=g)         # the diagonal: positives of the ME variant (distance ~1.7e-3 < 5e-3)
        if me:
            p2[:, 0] = p1[:, 0] + 0.3                              # row 0: no positive; row 1: three; rows 2, 3: none; the others: one
            p2[:, 2], p2[:, 3] = p1[:, 1] + 2e-3, p1[:, 1] - 2e-3
            p2[empty] = p1[empty] + 0.5
        else:
            p2[:, 1] = p1[:, 1] + 0.4                              # a diagonal pair farther than the threshold: still no negative
            p2[:, 3] = p1[:, 2]                                    # coincident off-diagonal points (2, 3): distance 0, not a negative
        d = torch.stack([_dist(p1[p], p2[p]) for p in range(P)])
        if not any((((d - f32(t)).abs() < 2e-4 * f32(t)).any()) for t in ((thr_pos, thr_neg) if me else (thr_neg,))):
            break
    if me:
        sim[:, 1, 2], sim[:, 1, 3] = sim[:, 1, 1] - 0.02, sim[:, 1, 1] + 0.015        # row 1's three positives within each other's active zone
    eye = torch.eye(N, dtype=torch.bool)
    for p in range(P):
        posm = (d[p] < f32(thr_pos)) if me else eye
        for _ in range(4):
            bad = _near_clamp(sim[p], posm, temp)
            if not bad.any():
                break
            low = torch.where(posm, sim[p], torch.full_like(sim[p], 2.0)).min(1).values.clamp(max=1.0)
            sim[p][bad] = (low[:, None] - 0.6).expand(N, N)[bad]
    return ApInputs(sim, p1, p2, None if counts is None else torch.tensor(counts, dtype=torch.int32), thr_pos, thr_neg, temp)


def ambiguous_ap(inp, me=False, rel=1e-4):
    """distances within a relative `rel` of a threshold + sigmoid exponents within a relative `rel` of the clamp, inside counts."""
    bad = 0
    inv = inv_temp(inp.temp)
    for p in range(inp.sim.shape[0]):
        n = inp.n(p)
        d = _dist(inp.p1[p, :n], inp.p2[p, :n])
        for thr in ((inp.thr_pos, inp.thr_neg) if me else (inp.thr_neg,)):
            bad += int(((d - f32(thr)).abs() < rel * f32(thr)).sum())
        s = inp.sim[p, :n, :n].double()
        ii, jj = torch.nonzero(d < f32(inp.thr_pos), as_tuple=True) if me else (torch.arange(n), torch.arange(n))
        pos = s[ii, jj]
        for x in (s - 1.0, 1.0 - pos, s[ii] - pos[:, None]):
            bad += int((((x * inv).abs() - 50.0).abs() < 50.0 * rel).sum())
    return bad


def combine_inputs():
    g = torch.Generator().manual_seed(5000)
    P, N = 3, 5
    return (torch.randn(P, 2, N, 128, generator=g), torch.randn(P, 2, N, 128, generator=g), torch.randn(2 * P, HG, generator=g),
            torch.randn(P, HG, generator=g), torch.randn(P, generator=g), torch.tensor([0.7, 0.0, -1.3]))


def transpose_inputs():
    g = torch.Generator().manual_seed(5001)
    return torch.randn(2, 33, 65, generator=g), torch.tensor([0.37, -2.5])


def pair_ratios(r, du_bound):
    """For every ordered pair (i, j) of a rank_set result r (want_pairs=True): its contribution |sc dz[i, j, k]| to du at the channel k where that is
    largest — it enters du_i[k] and du_j[k] alike — over the smaller of the two elements' bounds -> (ratio [n, n], valid [n, n])."""
    c = r["dz"].v.abs() * abs(r["sc"])
    k = c.argmax(-1)
    cm = c.gather(-1, k[..., None])[..., 0]
    cols = torch.arange(k.shape[1])[None, :].expand_as(k)
    return cm / torch.minimum(du_bound.gather(1, k), du_bound[cols, k]), r["valid"]
