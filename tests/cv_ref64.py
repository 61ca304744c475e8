"""fp64 restatement of the cost-volume KL kernels (csrc/cost_volume.hip), three input families, the per-element error bounds
tests/test_gpu_cost_volume_paths.py holds the kernels to, and deliberately WRONG restatements (mutants) that tests/test_cv_ref_host.py uses to
show that the bounds are not vacuous.  Plain torch, CPU, fp64, no autograd in a checked formula.  A test helper, not a test module.

The operation, per pair and direction d (d = 0: rows of view 1 against columns of view 2 with t1, m1; d = 1: the reverse), as the kernels factor it:
  inv_i = 1 / max(||f_i||, 1e-12)        S_ij = inv_i inv_j <f_i, f_j>
  rowsum_i = max(sum_j T_ij, 1e-8)        t_ij = max(T_ij / rowsum_i, 1e-8)      W_i = sum_j t_ij      A_i = sum_j t_ij log t_ij
  logZ_i = log sum_j exp S_ij             B_i = sum_j t_ij S_ij                  row_i = A_i - B_i + W_i logZ_i   (kept rows)
  masked rows: row_i = 0 (vggt) | hw 1e-8 log(1e-8 hw) (mast3r)                  loss = 0.5 (sum of both directions' rows) / hw
  backward, a function of the GIVEN stats = {inv, rowsum, logZ, W} (the kernels read logZ and W, they do not recompute them):
  G_ij = coef ( keep1_i (W1_i exp(S_ij - logZ1_i) - t1_ij) + keep2_j (W2_j exp(S_ij - logZ2_j) - t2_ji) ),  coef = dloss / (2 hw)
  da^_i = sum_j G_ij inv_j f2_j,  db^_j = sum_i G_ij inv_i f1_i,  df_i = inv_i da^_i - f_i inv_i^3 <f_i, da^_i>

Operand kinds (KINDS).  f32 and bf16: the features are the MFMA operands as stored.  f16 (the tf32h engine): fp32 master features, S and the G
contractions from their fp16 copies, inverse norms of the fp32 rows (given to the kernel), the normalisation backward on the fp32 rows.  The
reference always computes from the operands the engine reads, so no operand rounding enters a bound; 16-bit products are exact in fp32.  x3 (the
wrapper's split engine): fp32 x = hi + lo + r, hi = bf16(x), lo = bf16(x - hi), |r| <= 2^-18 |x|, the lo lo product dropped: charged as
U_X3 = 2^-17 per operand on the score (`split_slack`), the reference staying on the fp32 features.

Notation of the bounds.  U = 2^-24.  An MFMA chain of n products is charged ACC n U sum|products| (ACC = 2 roundings per term: the matrix unit's
adder is not documented to round to nearest after every term).  __expf / exp2, __logf, logf, v_rcp: 2 U each (__logf absolute 2 U max(|log x|, 1):
it is a scaled v_log).  Every output's first-order bound is multiplied ONCE by SECOND = 2 for the dropped higher-order terms.  None is tuned.
  e_inv   (cv_norm_kernel) sum of C squares in any order, sqrtf, one division: relative (C / 2 + 6) U;  0 when the caller gives inv (prenorm)
  e_s(i, j) = (2 e_inv + 6 U) |S_ij| + ACC C U inv_i inv_j sum_c |f_ic f_jc|     (the persistent kernels' log2-domain constant and products: 6 U)
  NT = ceil(hw / 64) + 7: depth of a teacher row sum (per-lane chain, six wave levels);  e_rs = NT U relative (T >= 0, asserted by make_inputs)
  e_t = (NT + 5) U relative: rowsum, its reciprocal, the product, the fp32 constant 1e-8f (|1e-8f - 1e-8| < U 1e-8); 5 U when rowsum is given
  W: sum_j t (e_t + NT U)        A: sum_j ( (|log t| + 1) t e_t + 2 U t max(|log t|, 1) + NT U |t log t| )
  NS = 24 + tiles: depth of a Z or B sum (lane chain, 16-lane row sum, wave halves, slabs).  The persistent kernels add exp2(0) = 1 for every
  entry past the ragged edge and subtract the count: Z is charged NS U (Z + 2 npad), npad = 128 tiles - hw.
  logZ: ( sum_j e^S (e_s + 2 U) + NS U (Z + 2 npad) ) / Z + 2 U |logZ|
  B: sum_j t ( |S| (e_t + (NS + 6) U) + e_s )        row: eA + eB + eW |logZ| + W e_logZ + 3 U (|A| + |B| + |W logZ|)
  loss: 0.5 / hw sum of the kept rows' bounds + 5 U |masked constant| per masked row + U |loss|   (the double accumulation is not charged)
  G (e_inv = 0: inv is part of the given stats), per direction  pt = W exp(S - logZ) (relative e_s + 2 U (|S| + |logZ|) + 8 U: the exponent's
  subtraction or the log2 constants, exp, products), t (relative 7 U), then 6 U (sum of all four terms) for the additions and coef;
  the store of G inv: U + u_T per direction's |pt - t| (the kept-row backward rounds each direction by itself), fp16: + 2^-25 / scale absolute
  below the normal range (scale: cv_gscale_kernel's power of two); the contractions ACC max(hwp, kcap) U + 2 U (scatter add);
  cv_norm_bwd: dot of C terms (C / 64 + 10) U, inv^3 and the products 4 U, the output 3 U, then the store's rounding (bf16 df).
Not bounded from code: gd_gemm_nt's f32 path is taken to be an fp32 MFMA accumulation (ACC per term, like every other chain)."""
import math

import torch

U = 2.0 ** -24
SECOND = 2.0
ACC = 2.0
EPS = 1e-8
U_X3 = 2.0 ** -17
PREC = {torch.float32: 24, torch.float16: 11, torch.bfloat16: 8}
EMIN = {torch.float32: -126, torch.float16: -14, torch.bfloat16: -126}
# name -> (operand dtype, C ABI dtype code, u_T of a stored G / df element)
KINDS = {"f32": (torch.float32, 0, 0.0), "bf16": (torch.bfloat16, 1, 2.0 ** -9), "f16": (torch.float16, 3, 2.0 ** -12)}
FAMILIES = ("random", "exact", "selector")
VARIANTS = ("vggt", "mast3r")
SELECT_ROWS = (0, 63, 64, 127, 128, -1)


def half_ulp(v, dtype):
    _, e = torch.frexp(v.abs().double())
    e = torch.where(v == 0, torch.full_like(e, EMIN[dtype]), torch.clamp(e - 1, min=EMIN[dtype]))
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - PREC[dtype])


def tiles(hw):
    return (hw + 127) // 128


def hwp(hw):
    return (hw + 63) // 64 * 64


def gscale(gloss, hw):
    """cv_gscale_kernel: the power of two the fp16 G is stored under."""
    m = float(gloss.abs().max()) * 0.5 / hw
    s = 2.0 ** math.floor(math.log2(4096.0 / m)) if 0.0 < m < 3.0e38 else 1.0
    return min(max(s, 1.0), 7.9e28)


# ------------------------------------------------------------------------------------------------ inputs
class Inputs:
    """f1, f2 [P, hw, C] fp32 masters (exactly representable in the kind's operand type unless kind = f16 and family = random), t1, t2 [P, hw, hw]
    fp32, m1, m2 [P, hw] bool, gloss [P] fp32."""

    def __init__(self, f1, f2, t1, t2, m1, m2, gloss, kind, family):
        self.f1, self.f2, self.t1, self.t2, self.m1, self.m2, self.gloss, self.kind, self.family = f1, f2, t1, t2, m1, m2, gloss, kind, family
        self.P, self.hw, self.C = f1.shape
        assert float(t1.min()) >= 0.0 and float(t2.min()) >= 0.0

    def operands(self):
        """the tensors the engine's MFMAs read, in their own dtype"""
        dt = KINDS[self.kind][0]
        return self.f1.to(dt), self.f2.to(dt)

    def inv32(self):
        """fp32 inverse norms of the master rows, as a producer would hand them over (..._prenorm)"""
        return tuple((1.0 / f.double().norm(dim=-1).clamp_min(1e-12)).float() for f in (self.f1, self.f2))


def _exact_rows(g, P, hw, C, kmin, kmax):
    M = min(C, 7)
    m = torch.randint(0, M, (P, hw), generator=g)
    sign = (torch.randint(0, 2, (P, hw), generator=g) * 2 - 1).float()
    k = torch.randint(kmin, kmax + 1, (P, hw), generator=g).float()
    f = torch.zeros(P, hw, C)
    f.scatter_(2, m[..., None], (sign * torch.exp2(k))[..., None])
    return f


def _perm(hw):
    a = next(a for a in range(5, hw + 6) if math.gcd(a, hw) == 1) if hw > 1 else 1
    return (torch.arange(hw) * a + 37) % hw


def select_rows(hw, P):
    """row kept by (pair p, view d) of the selector probe"""
    cand = sorted({r if r >= 0 else hw - 1 for r in SELECT_ROWS if r < hw})
    return [[cand[(2 * p + d) % len(cand)] for d in range(2)] for p in range(P)]


def make_inputs(family, P, hw, C, kind, seed=None):
    g = torch.Generator().manual_seed(1000 * hw + C if seed is None else seed)
    dt = KINDS[kind][0]
    kr = (0, 6) if kind == "f16" else (-8, 8)          # fp16: norms >= 1 keep G inv inside fp16's range under cv_gscale's scale
    gl = torch.tensor([1.0, -1e-4, 0.0, 1e-2, 3.0, 1e2])[:P].clone() if P > 1 else torch.tensor([0.37])
    if family == "random":
        r = min(4, C)
        basis = torch.randn(r, C, generator=g)
        fs = []
        for _ in range(2):
            w = torch.randn(P, hw, r, generator=g) * torch.tensor([3.0, 1.0, 0.5, 0.25][:r])
            f = w @ basis + 0.3 * torch.randn(P, hw, C, generator=g)
            f = f / f.norm(dim=-1, keepdim=True)
            dec = torch.rand(P, hw, 1, generator=g) * (1.5 if kind == "f16" else 4.0) - (0.0 if kind == "f16" else 2.0)
            fs.append((f * 10.0 ** dec).to(dt).float() if kind != "f16" else (f * 10.0 ** dec))
        f1, f2 = fs
        if hw > 2:
            f1[0, 1] = 0.0                                 # exactly zero feature rows
            f2[P - 1, hw - 2] = 0.0
        t1 = torch.softmax(3 * torch.randn(P, hw, hw, generator=g), -1)
        t2 = torch.softmax(3 * torch.randn(P, hw, hw, generator=g), -1)
        if hw > 4:
            t1[0, 3] = 0.0                                 # rowsum clamp
            t2[0, 2] = 0.0
            t2[0, 2, hw // 2] = 0.25                       # a single nonzero entry
            t1[P - 1, 4, :hw // 2] *= 1e-9                 # entries below the 1e-8 clamp after normalisation
        m1 = torch.rand(P, hw, generator=g) > 0.3
        m2 = torch.rand(P, hw, generator=g) > 0.3
        m2[0] = False                                      # one view of one pair fully masked
        m1[P - 1] = True                                   # one pair fully kept
        m2[P - 1] = True
        return Inputs(f1, f2, t1, t2, m1, m2, gl, kind, family)
    f1, f2 = _exact_rows(g, P, hw, C, *kr), _exact_rows(g, P, hw, C, *kr)
    if family == "exact":
        t1 = torch.softmax(3 * torch.randn(P, hw, hw, generator=g), -1)
        t2 = torch.softmax(3 * torch.randn(P, hw, hw, generator=g), -1)
        m1 = torch.rand(P, hw, generator=g) > 0.3
        m2 = torch.rand(P, hw, generator=g) > 0.3
        m1[0, 0] = m2[0, hw - 1] = True
        return Inputs(f1, f2, t1, t2, m1, m2, gl, kind, family)
    assert family == "selector"
    pi = _perm(hw)
    t = torch.zeros(hw, hw)
    t[torch.arange(hw), pi] = 1.0
    t1, t2 = t.expand(P, hw, hw).contiguous(), t.expand(P, hw, hw).contiguous()
    m1, m2 = torch.zeros(P, hw, dtype=torch.bool), torch.zeros(P, hw, dtype=torch.bool)
    for p, (r1, r2) in enumerate(select_rows(hw, P)):
        m1[p, r1] = m2[p, r2] = True
        # the selected score is +-1, never 0: the selected column carries the kept row's axis (view 2's kept row is settled first, then view 1's)
        ax1 = int(f1[p, r1].abs().argmax())
        f2[p, pi[r1]] = 0.0
        f2[p, pi[r1], ax1] = -2.0 ** kr[0] if (p + r1) % 2 else 2.0 ** kr[1]
        ax2 = int(f2[p, r2].abs().argmax())
        if int(pi[r2]) != r1:
            f1[p, pi[r2]] = 0.0
            f1[p, pi[r2], ax2] = 2.0 ** kr[0] if (p + r2) % 2 else -2.0 ** kr[1]
    gl = gl.clone()
    gl[gl == 0] = 0.5                                      # every pair's selected row shows in the gradients
    return Inputs(f1, f2, t1, t2, m1, m2, gl, kind, family)


# ------------------------------------------------------------------------------------------------ the restatement, with mutation hooks
class Mutant:
    """cw [hw]: multiplicity of every student column in Z (and in the backward's softmax term); bw [hw]: multiplicity of every teacher column in B;
    zadd: ones added to every Z (pad columns taken as live); gpad: pad columns of G that hold the last live column's value and meet the last feature
    row; flip = (p, d, row): that row's mask inverted; stats_roll: the backward reads pair p + 1's logZ and W; t_swap: direction 1 reads t1;
    inv_swap: S scaled by the other view's inverse norms; vggt_const: the masked rows' constant of vggt for mast3r; shift: direction 0's kept rows read
    the teacher row after their own."""

    def __init__(self, name, **kw):
        self.name = name
        self.cw = self.bw = self.flip = None
        self.zadd = self.gpad = 0
        self.stats_roll = self.t_swap = self.inv_swap = self.vggt_const = self.shift = False
        for k, v in kw.items():
            assert hasattr(self, k)
            setattr(self, k, v)


def mutants(x):
    """-> [(name, Mutant or None)]; None where the mutant IS the reference for these inputs (the host test asserts which)."""
    P, hw = x.P, x.hw
    ones = torch.ones(hw, dtype=torch.float64)

    def one(j, w):
        t = ones.clone()
        t[j] = w
        return t
    # a kept row of direction 0 in pair 0 and its heaviest teacher column: where a dropped column shows
    kept = torch.nonzero(x.m1[0])
    i0 = int(kept[0]) if len(kept) else 0
    j0 = int(x.t1[0, i0].argmax())
    tile = ones.clone()
    t0 = (j0 // 128) * 128
    tile[t0:t0 + 128] = 0.0
    masked = [(p, d, int(torch.nonzero(~m[p])[0])) for p in range(P) for d, m in ((0, x.m1), (1, x.m2)) if bool((~m[p]).any())]
    keptl = [(p, d, int(torch.nonzero(m[p])[0])) for p in range(P) for d, m in ((0, x.m1), (1, x.m2)) if bool(m[p].any())]
    npad, gp = tiles(hw) * 128 - hw, hwp(hw) - hw
    return [("drop_student_col", Mutant("drop_student_col", cw=one(j0, 0.0)) if hw > 1 else None),
            ("double_student_col", Mutant("double_student_col", cw=one(j0, 2.0))),
            ("drop_teacher_col_B", Mutant("drop_teacher_col_B", bw=one(j0, 0.0))),
            ("skip_128_tile", Mutant("skip_128_tile", cw=tile) if hw > 128 else None),
            ("ragged_col_live", Mutant("ragged_col_live", zadd=1) if npad else None),
            ("G_pad_nonzero", Mutant("G_pad_nonzero", gpad=gp) if gp else None),
            ("masked_as_kept", Mutant("masked_as_kept", flip=masked[0]) if masked else None),
            ("kept_as_masked", Mutant("kept_as_masked", flip=keptl[0]) if keptl else None),
            ("neighbour_pair_stats", Mutant("neighbour_pair_stats", stats_roll=True) if P > 1 else None),
            ("t1_for_direction_2", Mutant("t1_for_direction_2", t_swap=True) if hw > 1 else None),
            ("inv_of_other_view", Mutant("inv_of_other_view", inv_swap=True) if hw > 1 else None),
            ("vggt_const_for_mast3r", Mutant("vggt_const_for_mast3r", vggt_const=True) if masked else None),
            ("kept_index_off_by_one", Mutant("kept_index_off_by_one", shift=True) if hw > 1 else None)]


def _masks(x, mut):
    m1, m2 = x.m1.clone(), x.m2.clone()
    if mut is not None and mut.flip is not None:
        p, d, r = mut.flip
        (m2 if d else m1)[p, r] = ~(m2 if d else m1)[p, r]
    return m1, m2


def _scores(fa, fb, inv1, inv2, mut):
    if mut is not None and mut.inv_swap:
        inv1, inv2 = inv2, inv1
    dots, absd = fa @ fb.transpose(-1, -2), fa.abs() @ fb.abs().transpose(-1, -2)
    sc = inv1[:, :, None] * inv2[:, None, :]
    return sc * dots, sc * absd


def _teacher(T, rs=None):
    if rs is None:
        rs = T.sum(-1).clamp_min(EPS)
    return rs, (T / rs[..., None]).clamp_min(EPS)


def teacher_stats64(x):
    """gd_cost_volume_teacher_stats -> (tstats [P, 2, hw, 4] fp64 = {rowsum, W, A, 0}, bound of the same shape)"""
    hw = x.hw
    NT = (hw + 63) // 64 + 7
    e_t = (NT + 5) * U
    out, bnd = [], []
    for T in (x.t1.double(), x.t2.double()):
        rs, t = _teacher(T)
        lt = t.log()
        W, A = t.sum(-1), (t * lt).sum(-1)
        eW = (t * (e_t + NT * U)).sum(-1)
        eA = ((lt.abs() + 1) * t * e_t + 2 * U * t * lt.abs().clamp_min(1.0) + NT * U * (t * lt).abs()).sum(-1)
        out.append(torch.stack([rs, W, A, torch.zeros_like(W)], -1))
        bnd.append(torch.stack([SECOND * NT * U * rs, SECOND * eW, SECOND * eA, torch.zeros_like(W)], -1))
    return torch.stack(out, 1), torch.stack(bnd, 1)


def forward64(x, variant, inv=None, tstats=None, mut=None, split_slack=0.0):
    """-> dict: loss [P], stats [P, 2, hw, 4] = {inv, rowsum, logZ, W}, rows [P, 2, hw], B, and the bounds b_loss, b_stats.
    inv = (inv1, inv2) GIVEN to the kernel (fp32 tensors, ..._prenorm) or None (cv_norm_kernel); tstats [P, 2, hw, 4] GIVEN or None."""
    fa, fb = [t.double() for t in x.operands()]
    if split_slack:
        fa, fb = x.f1.double(), x.f2.double()
    P, hw, C = x.P, x.hw, x.C
    if inv is None:
        inv1, inv2 = [1.0 / f.norm(dim=-1).clamp_min(1e-12) for f in (fa, fb)]
        e_inv = (C / 2 + 6) * U
    else:
        inv1, inv2 = inv[0].double(), inv[1].double()
        e_inv = 0.0
    S, Sabs = _scores(fa, fb, inv1, inv2, mut)
    e_s = (2 * e_inv + 6 * U + 2 * split_slack) * S.abs() + (ACC * C * U + 2 * split_slack) * Sabs
    m1, m2 = _masks(x, mut)
    NT, NS, npad = (hw + 63) // 64 + 7, 24 + tiles(hw), tiles(hw) * 128 - hw
    const = hw * EPS * math.log(EPS * hw) if (variant == "mast3r" and not (mut is not None and mut.vggt_const)) else 0.0
    stats, bstats, rows, brows, Bs = [], [], [], [], []
    for d in range(2):
        Sd, esd = (S, e_s) if d == 0 else (S.transpose(-1, -2), e_s.transpose(-1, -2))
        T = (x.t1 if d == 0 or (mut is not None and mut.t_swap) else x.t2).double()
        if mut is not None and mut.shift and d == 0:
            T = T.roll(-1, dims=1)
        if tstats is None:
            rs, t = _teacher(T)
            lt = t.log()
            W, A = t.sum(-1), (t * lt).sum(-1)
            e_t = (NT + 5) * U
            eW = (t * (e_t + NT * U)).sum(-1)
            eA = ((lt.abs() + 1) * t * e_t + 2 * U * t * lt.abs().clamp_min(1.0) + NT * U * (t * lt).abs()).sum(-1)
            e_rs = NT * U * rs
        else:
            rs, W, A = [tstats[:, d, :, k].double() for k in range(3)]
            _, t = _teacher(T, rs)
            e_t, eW, eA, e_rs = 5 * U, torch.zeros_like(W), torch.zeros_like(W), torch.zeros_like(W)
        E = Sd.exp()
        cw = mut.cw if mut is not None and mut.cw is not None else None
        Z = (E * cw).sum(-1) if cw is not None else E.sum(-1)
        if mut is not None:
            Z = Z + mut.zadd
        logZ = Z.log()
        e_logZ = ((E * (esd + 2 * U)).sum(-1) + NS * U * (Z + 2 * npad)) / Z + 2 * U * logZ.abs()
        ts = t * Sd
        B = (ts * mut.bw).sum(-1) if mut is not None and mut.bw is not None else ts.sum(-1)
        eB = (t * (Sd.abs() * (e_t + (NS + 6) * U) + esd)).sum(-1)
        row = A - B + W * logZ
        e_row = eA + eB + eW * logZ.abs() + W * e_logZ + 3 * U * (A.abs() + B.abs() + (W * logZ).abs())
        keep = (m1, m2)[d]
        rows.append(torch.where(keep, row, torch.full_like(row, const)))
        brows.append(torch.where(keep, e_row, torch.full_like(row, 5 * U * abs(const))))
        Bs.append(B)
        iv = (inv1, inv2)[d]
        stats.append(torch.stack([iv, rs, logZ, W], -1))
        bstats.append(torch.stack([SECOND * e_inv * iv, SECOND * e_rs, SECOND * e_logZ, SECOND * eW], -1))
    rows, brows = torch.stack(rows, 1), torch.stack(brows, 1)
    loss = 0.5 * rows.sum((1, 2)) / hw
    b_loss = SECOND * 0.5 * brows.sum((1, 2)) / hw + U * loss.abs()
    return {"loss": loss, "b_loss": b_loss, "stats": torch.stack(stats, 1), "b_stats": torch.stack(bstats, 1), "rows": rows, "B": torch.stack(Bs, 1)}


def backward64(x, stats, mut=None, kcap=0):
    """-> (df1, df2, b_df1, b_df2) [P, hw, C] for the GIVEN stats [P, 2, hw, 4] (any float tensor).  kcap: the kept-row backward's capacity (its
    contraction length enters the bound), 0 for the dense backward."""
    fa, fb = [t.double() for t in x.operands()]
    P, hw, C = x.P, x.hw, x.C
    st = stats.double()
    inv1, inv2 = st[:, 0, :, 0], st[:, 1, :, 0]
    S, Sabs = _scores(fa, fb, inv1, inv2, mut)
    e_s = 6 * U * S.abs() + ACC * C * U * Sabs
    m1, m2 = _masks(x, mut)
    coef = (x.gloss.double() * 0.5 / hw)[:, None, None]
    lw = st.roll(-1, dims=0) if mut is not None and mut.stats_roll else st
    G, eG, Gd = 0.0, 0.0, 0.0
    for d in range(2):
        tr = (lambda a: a) if d == 0 else (lambda a: a.transpose(-1, -2))
        T = (x.t1 if d == 0 or (mut is not None and mut.t_swap) else x.t2).double()
        if mut is not None and mut.shift and d == 0:
            T = T.roll(-1, dims=1)
        _, t = _teacher(T, st[:, d, :, 1])
        logZ, W = lw[:, d, :, 2][..., None], lw[:, d, :, 3][..., None]
        Sd, esd = tr(S), tr(e_s)
        pt = W * (Sd - logZ).exp()
        if mut is not None and mut.cw is not None:
            pt = pt * mut.cw
        keep = (m1, m2)[d][..., None]                  # a select, as in the kernels: a masked row's logZ and W may be anything (NaN included)
        zero = torch.zeros((), dtype=torch.float64)
        rel = esd + 2 * U * (Sd.abs() + logZ.abs()) + 8 * U
        G = G + tr(torch.where(keep, pt - t, zero))
        eG = eG + tr(torch.where(keep, pt.abs() * rel + t * 7 * U + 6 * U * (pt.abs() + t), zero))
        Gd = Gd + tr(torch.where(keep, (pt - t).abs(), zero))
    G, eG, Gd = coef * G, coef.abs() * eG, coef.abs() * Gd
    u_T = KINDS[x.kind][2]
    sub = (2.0 ** -25 / gscale(x.gloss, hw)) * (coef != 0).double() if x.kind == "f16" else 0.0
    K = max(hwp(hw), kcap)
    f1m, f2m = (x.f1.double(), x.f2.double()) if x.kind == "f16" else (fa, fb)
    out = []
    for d in range(2):
        tr = (lambda a: a) if d == 0 else (lambda a: a.transpose(-1, -2))
        io, fo, fm, iv = ((inv2, fb, f1m, inv1), (inv1, fa, f2m, inv2))[d]      # the OTHER view's inv and operand rows; this view's master rows and inv
        G1 = tr(G) * io[:, None, :]
        e_G1 = tr(eG) * io[:, None, :] + tr(Gd) * io[:, None, :] * (U + u_T) + sub
        dah = G1 @ fo
        if mut is not None and mut.gpad:
            dah = dah + mut.gpad * G1[:, :, -1:] * fo[:, -1:, :]
        absc = (tr(Gd) * io[:, None, :]) @ fo.abs()
        e_dah = e_G1 @ fo.abs() + (ACC * K + 2) * U * absc
        iv1 = iv[..., None]
        dot = (fm * dah).sum(-1, keepdim=True)
        adot = (fm * dah).abs().sum(-1, keepdim=True)
        e_dot = (fm.abs() * e_dah).sum(-1, keepdim=True) + (C / 64 + 10) * U * adot
        e_k = iv1 ** 3 * (e_dot + 4 * U * adot)
        df = iv1 * dah - fm * iv1 ** 3 * dot
        b = SECOND * (iv1 * e_dah + fm.abs() * e_k + 3 * U * (iv1 * dah.abs() + fm.abs() * iv1 ** 3 * dot.abs()))
        if x.kind == "bf16":
            b = b + half_ulp(df.abs() + b, torch.bfloat16)
        out.append((df, b))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def ratio(got, ref, bound):
    """-> (worst err / bound, index); NaN or infinity anywhere is an infinite ratio; bound 0 demands equality."""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    if r.numel() == 0:
        return 0.0, ()
    i = int(r.argmax())
    return float(r.reshape(-1)[i]), tuple(int(t) for t in torch.unravel_index(torch.tensor(i), r.shape))
