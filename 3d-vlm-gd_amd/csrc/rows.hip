// The VGGT teacher's camera head (vggt/heads/camera_head.py) on a handful of token rows, M = B * S <= 8: a few-row linear that streams its weights
// once, attention among the S rows of a batch entry at any head dimension up to 256, the adaLN modulation and the pose update.  teacher_heads.
// FusedCameraHead chains them with gd_layernorm_fwd.
//
// gd_rows_linear is a weight-streaming kernel: at M <= 8 a linear layer is 2 M flops per weight byte pair, bandwidth-bound by more than an order of
// magnitude, and gd_gemm_nt's 128 x 128 MFMA tiles occupy N / 128 workgroups with 126 dead rows each.  Here
//   * x (with the SiLU prologue applied) is staged ONCE per workgroup in LDS, M * K floats;
//   * a wave owns RL_CPW output columns; its lanes walk K in 16-byte pieces of the weight rows, loaded straight from global memory to VGPRs
//     (non-temporal: every weight is read once per call), RL_UNROLL steps of RL_CPW loads in flight before the first is used; W never sees LDS;
//   * every (row, column) has ONE accumulator per lane, a single fmaf chain in increasing k, and the 64 lane sums meet in wave_sum's fixed DPP tree:
//     the summation order of an output element depends on K and the weight type alone — not on M, N, the grid or the column's place in its wave.  No
//     split-K across waves, no atomics;
//   * lane m * RL_CPW + c of the wave then applies the epilogue of element (m, column c) and stores it: bias, exact GELU, gamma * v + residual.
#include "gd_common.h"

#define RL_CPW 2            // output columns per wave
#define RL_WAVES 4          // waves per workgroup: RL_CPW * RL_WAVES = 8 columns per workgroup
#define RL_UNROLL 4         // K steps whose weight loads are issued before the first is consumed
#define RL_MAX_M 8
#define RL_LDS_FLOATS 16384 // the staged x: M * K <= 16384 floats = 64 KB (M <= 8 at K <= 2048, M <= 2 at K <= 8192)

struct RlArgs {
    const float* x;
    const void* w;
    float* y;
    const float *bias, *residual, *gamma;
    int N, K;
    long ldx, ldw, ldy, ldr;
    int prologue, act;
};

__device__ __forceinline__ float silu_f(float v) { return v / (1.0f + expf(-v)); }

// one 16-byte piece of a weight row as floats: 4 (fp32) or 8 (bf16) consecutive k
template <typename TW> struct RlPiece;
template <> struct RlPiece<float> {
    static constexpr int E = 4;
    typedef f32x4 Raw;
    static __device__ __forceinline__ void widen(Raw r, float (&f)[4]) { f[0] = r[0]; f[1] = r[1]; f[2] = r[2]; f[3] = r[3]; }
};
template <> struct RlPiece<bf16> {
    static constexpr int E = 8;
    typedef bf16x8 Raw;
    static __device__ __forceinline__ void widen(Raw r, float (&f)[8]) {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = (float)r[e];
    }
};

template <typename TW, int M> __global__ __launch_bounds__(64 * RL_WAVES) void rows_linear_kernel(RlArgs a) {
    extern __shared__ __attribute__((aligned(16))) float xs[];          // [M][K]
    typedef RlPiece<TW> P;
    constexpr int E = P::E;
    const int K = a.K, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // ---- stage x: K % 4 == 0, so a row is K / 4 whole 16-byte pieces
    const int q4 = K >> 2;
    for (int i = threadIdx.x; i < M * q4; i += 64 * RL_WAVES) {
        const int m = i / q4, c = (i - m * q4) * 4;
        f32x4 v = *(const f32x4*)(a.x + (long)m * a.ldx + c);
        if (a.prologue == 1) { v[0] = silu_f(v[0]); v[1] = silu_f(v[1]); v[2] = silu_f(v[2]); v[3] = silu_f(v[3]); }
        *(f32x4*)(xs + m * K + c) = v;
    }
    __syncthreads();
    const int n0 = (blockIdx.x * RL_WAVES + wave) * RL_CPW;
    if (n0 >= a.N) return;
    // a column past N (the last wave of an odd N) streams column N - 1 again and stores nothing
    const TW* wr[RL_CPW];
#pragma unroll
    for (int c = 0; c < RL_CPW; ++c) wr[c] = (const TW*)a.w + (long)min(n0 + c, a.N - 1) * a.ldw;
    float acc[M][RL_CPW];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int c = 0; c < RL_CPW; ++c) acc[m][c] = 0.f;

    auto consume = [&](const typename P::Raw (&raw)[RL_CPW], int k) {
        float wf[RL_CPW][E];
#pragma unroll
        for (int c = 0; c < RL_CPW; ++c) P::widen(raw[c], wf[c]);
#pragma unroll
        for (int m = 0; m < M; ++m) {
            float xf[E];
#pragma unroll
            for (int e = 0; e < E; e += 4) {
                const f32x4 xv = *(const f32x4*)(xs + m * K + k + e);
                xf[e] = xv[0]; xf[e + 1] = xv[1]; xf[e + 2] = xv[2]; xf[e + 3] = xv[3];
            }
#pragma unroll
            for (int c = 0; c < RL_CPW; ++c)
#pragma unroll
                for (int e = 0; e < E; ++e) acc[m][c] = fmaf(xf[e], wf[c][e], acc[m][c]);
        }
    };

    const int pieces = K / E, full = pieces >> 6;                        // steps in which all 64 lanes hold a piece
    int step = 0;
    for (; step + RL_UNROLL <= full; step += RL_UNROLL) {
        typename P::Raw raw[RL_UNROLL][RL_CPW];
#pragma unroll
        for (int u = 0; u < RL_UNROLL; ++u)
#pragma unroll
            for (int c = 0; c < RL_CPW; ++c)
                raw[u][c] = __builtin_nontemporal_load((const typename P::Raw*)(wr[c] + ((step + u) * 64 + lane) * E));
#pragma unroll
        for (int u = 0; u < RL_UNROLL; ++u) consume(raw[u], ((step + u) * 64 + lane) * E);
    }
    for (; step < full; ++step) {
        typename P::Raw raw[RL_CPW];
#pragma unroll
        for (int c = 0; c < RL_CPW; ++c) raw[c] = __builtin_nontemporal_load((const typename P::Raw*)(wr[c] + (step * 64 + lane) * E));
        consume(raw, (step * 64 + lane) * E);
    }
    if (full * 64 + lane < pieces) {                                     // the K tail: the first pieces % 64 lanes
        typename P::Raw raw[RL_CPW];
#pragma unroll
        for (int c = 0; c < RL_CPW; ++c) raw[c] = __builtin_nontemporal_load((const typename P::Raw*)(wr[c] + (full * 64 + lane) * E));
        consume(raw, (full * 64 + lane) * E);
    }
    // ---- the 64 lane sums of every element, then lane m * RL_CPW + c finishes element (m, c)
    float mine = 0.f;
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int c = 0; c < RL_CPW; ++c) {
            const float s = wave_sum(acc[m][c]);
            if (lane == m * RL_CPW + c) mine = s;
        }
    if (lane >= M * RL_CPW) return;
    const int m = lane / RL_CPW, n = n0 + lane % RL_CPW;
    if (n >= a.N) return;
    float v = mine;
    if (a.bias) v += a.bias[n];
    if (a.act == 1) v = gelu_f(v);
    if (a.residual) {
        const float r = a.residual[(long)m * a.ldr + n];
        v = a.gamma ? fmaf(a.gamma[n], v, r) : r + v;
    }
    a.y[(long)m * a.ldy + n] = v;
}

static bool rl_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}

template <typename TW> static void rl_launch(const RlArgs& a, int M, hipStream_t s) {
    const dim3 grid(gd_cdiv(a.N, RL_CPW * RL_WAVES)), blk(64 * RL_WAVES);
    const size_t lds = (size_t)M * a.K * sizeof(float);
    switch (M) {
#define RL_CASE(MM) case MM: hipLaunchKernelGGL((rows_linear_kernel<TW, MM>), grid, blk, lds, s, a); break
        RL_CASE(1); RL_CASE(2); RL_CASE(3); RL_CASE(4); RL_CASE(5); RL_CASE(6); RL_CASE(7); RL_CASE(8);
#undef RL_CASE
    }
}

extern "C" int gd_rows_linear(const float* x, const void* w, int w_dtype, float* y, int M, int N, int K, long ldx, long ldw, long ldy, const float* bias,
                              const float* residual, long ldr, const float* gamma, int prologue, int activation, void* stream) {
    GD_REQUIRE(M >= 1 && M <= RL_MAX_M, "gd_rows_linear: M = %d: 1 to %d rows are served", M, RL_MAX_M);
    GD_REQUIRE(N >= 1 && N <= (1 << 24), "gd_rows_linear: N = %d must be in [1, 2^24]", N);
    GD_REQUIRE(w_dtype == GD_F32 || w_dtype == GD_BF16, "gd_rows_linear: w_dtype %d: fp32 (%d) or bf16 (%d) weights are served", w_dtype, GD_F32, GD_BF16);
    const int kq = w_dtype == GD_BF16 ? 8 : 4;
    GD_REQUIRE(K >= kq && K % kq == 0, "gd_rows_linear: K = %d must be a positive multiple of %d for %s weights", K, kq, w_dtype == GD_BF16 ? "bf16" : "fp32");
    GD_REQUIRE((long)M * K <= RL_LDS_FLOATS, "gd_rows_linear: M * K = %d * %d = %ld exceeds the %d floats of x the kernel stages in LDS", M, K, (long)M * K,
               RL_LDS_FLOATS);
    GD_REQUIRE(ldx >= K && ldx % 4 == 0, "gd_rows_linear: ldx = %ld must be a multiple of 4 and >= K = %d", ldx, K);
    GD_REQUIRE(ldw >= K && ldw % kq == 0, "gd_rows_linear: ldw = %ld must be a multiple of %d and >= K = %d", ldw, kq, K);
    GD_REQUIRE(ldy >= N && ldy % 4 == 0, "gd_rows_linear: ldy = %ld must be a multiple of 4 and >= N = %d", ldy, N);
    GD_REQUIRE(prologue == 0 || prologue == 1, "gd_rows_linear: prologue %d: 0 (none) or 1 (SiLU)", prologue);
    GD_REQUIRE(activation == 0 || activation == 1, "gd_rows_linear: activation %d: 0 (none) or 1 (exact GELU)", activation);
    GD_REQUIRE(x && w && y, "gd_rows_linear: x, w and y are required");
    GD_REQUIRE(residual || !gamma, "gd_rows_linear: gamma is given without a residual");
    GD_REQUIRE(!residual || (ldr >= N && ldr % 4 == 0), "gd_rows_linear: ldr = %ld must be a multiple of 4 and >= N = %d", ldr, N);
    GD_REQUIRE((uintptr_t)x % 16 == 0, "gd_rows_linear: x %p must be 16-byte aligned", (const void*)x);
    GD_REQUIRE((uintptr_t)w % 16 == 0, "gd_rows_linear: w %p must be 16-byte aligned", w);
    GD_REQUIRE((uintptr_t)y % 16 == 0, "gd_rows_linear: y %p must be 16-byte aligned", (void*)y);
    GD_REQUIRE((uintptr_t)residual % 16 == 0, "gd_rows_linear: residual %p must be 16-byte aligned", (const void*)residual);
    GD_REQUIRE(((uintptr_t)bias | (uintptr_t)gamma) % 4 == 0, "gd_rows_linear: bias %p and gamma %p must be 4-byte aligned", (const void*)bias, (const void*)gamma);
    const size_t ybytes = ((size_t)(M - 1) * ldy + N) * 4, xbytes = ((size_t)(M - 1) * ldx + K) * 4;
    const size_t wbytes = ((size_t)(N - 1) * ldw + K) * gd_dtype_size(w_dtype);
    GD_REQUIRE(rl_disjoint(y, ybytes, x, xbytes), "gd_rows_linear: y [%p, +%zu) overlaps x [%p, +%zu)", (void*)y, ybytes, (const void*)x, xbytes);
    GD_REQUIRE(rl_disjoint(y, ybytes, w, wbytes), "gd_rows_linear: y [%p, +%zu) overlaps w [%p, +%zu)", (void*)y, ybytes, w, wbytes);
    if (residual) {
        const size_t rbytes = ((size_t)(M - 1) * ldr + N) * 4;
        // in place on the token stream: element (m, n) is read and written by one lane.  Any other intersection would be a race.
        GD_REQUIRE((residual == y && ldr == ldy) || rl_disjoint(y, ybytes, residual, rbytes),
                   "gd_rows_linear: y [%p, ld %ld] overlaps residual [%p, ld %ld] without being the same pointer and stride", (void*)y, ldy,
                   (const void*)residual, ldr);
    }
    RlArgs a;
    a.x = x; a.w = w; a.y = y; a.bias = bias; a.residual = residual; a.gamma = gamma;
    a.N = N; a.K = K; a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.ldr = ldr; a.prologue = prologue; a.act = activation;
    if (w_dtype == GD_BF16) rl_launch<bf16>(a, M, (hipStream_t)stream);
    else rl_launch<float>(a, M, (hipStream_t)stream);
    GD_LAUNCH_OK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// Attention among the S <= 8 rows of each batch entry (vggt/layers/attention.py:87-123 with rope=None, qk_norm=False): one wave per (entry, head,
// query row); lane t holds q[4t .. 4t+3] and accumulates output columns 4t .. 4t+3 (lanes with 4t >= hd idle); a score is four fmaf and one wave
// sum; softmax in exact fp32 with the maximum subtracted (expf).
#define RA_MAX_S 8
#define RA_MAX_HD 256

__global__ __launch_bounds__(256) void rows_attention_kernel(const float* qkv, float* o, int B, int S, int H, int hd, long ld, long ldo, float scale) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);         // (b, h, i)
    if (row >= (long)B * H * S) return;
    const int i = (int)(row % S), h = (int)((row / S) % H), b = (int)(row / ((long)S * H));
    const int W = H * hd;
    const bool active = 4 * lane < hd;
    const long col = (long)h * hd + 4 * lane;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const float* base = qkv + (long)b * S * ld + col;
    const f32x4 q = active ? *(const f32x4*)(base + (long)i * ld) : zero;
    float s[RA_MAX_S];
    f32x4 v[RA_MAX_S];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < RA_MAX_S; ++j) {
        if (j < S) {
            const f32x4 k = active ? *(const f32x4*)(base + (long)j * ld + W) : zero;
            v[j] = active ? *(const f32x4*)(base + (long)j * ld + 2 * W) : zero;
            float d = q[0] * k[0];
            d = fmaf(q[1], k[1], d);
            d = fmaf(q[2], k[2], d);
            d = fmaf(q[3], k[3], d);
            s[j] = wave_sum(d) * scale;
            mx = fmaxf(mx, s[j]);
        }
    }
    float l = 0.f;
    f32x4 acc = zero;
#pragma unroll
    for (int j = 0; j < RA_MAX_S; ++j) {
        if (j < S) {
            const float p = expf(s[j] - mx);
            l += p;
            acc[0] = fmaf(p, v[j][0], acc[0]);
            acc[1] = fmaf(p, v[j][1], acc[1]);
            acc[2] = fmaf(p, v[j][2], acc[2]);
            acc[3] = fmaf(p, v[j][3], acc[3]);
        }
    }
    if (active) {
        f32x4 r;
        r[0] = acc[0] / l; r[1] = acc[1] / l; r[2] = acc[2] / l; r[3] = acc[3] / l;
        *(f32x4*)(o + ((long)b * S + i) * ldo + col) = r;
    }
}

extern "C" int gd_rows_attention(const float* qkv, float* o, int B, int S, int H, int head_dim, long ld, long ldo, float scale, void* stream) {
    GD_REQUIRE(S >= 1 && S <= RA_MAX_S, "gd_rows_attention: S = %d: 1 to %d rows per batch entry are served", S, RA_MAX_S);
    GD_REQUIRE(head_dim >= 4 && head_dim <= RA_MAX_HD && head_dim % 4 == 0, "gd_rows_attention: head_dim %d: a multiple of 4 from 4 to %d is served", head_dim,
               RA_MAX_HD);
    GD_REQUIRE(B >= 1 && H >= 1 && (long)B * S * H < (1L << 30) && (long)H * head_dim < (1L << 28), "gd_rows_attention: need B, H >= 1 within the grid (B=%d H=%d)", B, H);
    const long W = (long)H * head_dim;
    GD_REQUIRE(ld >= 3 * W && ld % 4 == 0, "gd_rows_attention: ld = %ld must be a multiple of 4 and >= 3 * H * head_dim = %ld", ld, 3 * W);
    GD_REQUIRE(ldo >= W && ldo % 4 == 0, "gd_rows_attention: ldo = %ld must be a multiple of 4 and >= H * head_dim = %ld", ldo, W);
    GD_REQUIRE(qkv && o, "gd_rows_attention: qkv and o are required");
    GD_REQUIRE((((uintptr_t)qkv | (uintptr_t)o) & 15) == 0, "gd_rows_attention: qkv %p and o %p must be 16-byte aligned", (const void*)qkv, (void*)o);
    const long rows = (long)B * S;
    GD_REQUIRE(rl_disjoint(o, (size_t)((rows - 1) * ldo + W) * 4, qkv, (size_t)((rows - 1) * ld + 3 * W) * 4), "gd_rows_attention: o overlaps qkv");
    hipLaunchKernelGGL(rows_attention_kernel, dim3((unsigned)gd_cdiv(rows * H, 4)), dim3(256), 0, (hipStream_t)stream, qkv, o, B, S, H, head_dim, ld, ldo, scale);
    GD_LAUNCH_OK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// camera_head.py:130-134: out = gate * (LN0(x) * (1 + scale) + shift) + x, LN0 without affine parameters; one wave per row, the row in registers
// (norm.hip's two-reduction body: mean, then the centred sum of squares).
#define AM_MAX_D 8192

template <int NV> __global__ __launch_bounds__(256) void adaln_modulate_kernel(const float* x, const float* mod, float* out, int M, int D, long ldx, long ldm,
                                                                               long ldo, float eps) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const float* xr = x + (long)row * ldx;
    f32x4 v[NV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < D) {
            v[i] = *(const f32x4*)(xr + c);
            s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
        }
    }
    const float mu = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < D) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { const float d = v[i][k] - mu; q += d * d; }
        }
    }
    const float rs = rsqrtf(wave_sum(q) / (float)D + eps);
    const float* mr = mod + (long)row * ldm;
    float* orow = out + (long)row * ldo;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < D) {
            const f32x4 sh = *(const f32x4*)(mr + c), sc = *(const f32x4*)(mr + D + c), g = *(const f32x4*)(mr + 2 * D + c);
            f32x4 r;
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k] = g[k] * ((v[i][k] - mu) * rs * (1.0f + sc[k]) + sh[k]) + v[i][k];
            *(f32x4*)(orow + c) = r;
        }
    }
}

extern "C" int gd_adaln_modulate(const float* x, const float* mod, float* out, int M, int D, long ldx, long ldm, long ldo, float eps, void* stream) {
    GD_REQUIRE(D >= 4 && D % 4 == 0 && D <= AM_MAX_D, "gd_adaln_modulate: D = %d must be a multiple of 4 from 4 to %d", D, AM_MAX_D);
    GD_REQUIRE(M >= 1, "gd_adaln_modulate: M = %d must be >= 1", M);
    GD_REQUIRE(ldx >= D && ldx % 4 == 0 && ldo >= D && ldo % 4 == 0 && ldm >= 3L * D && ldm % 4 == 0,
               "gd_adaln_modulate: strides ldx = %ld, ldo = %ld (>= D) and ldm = %ld (>= 3 D) must be multiples of 4 (D = %d)", ldx, ldo, ldm, D);
    GD_REQUIRE(x && mod && out, "gd_adaln_modulate: x, mod and out are required");
    GD_REQUIRE((((uintptr_t)x | (uintptr_t)mod | (uintptr_t)out) & 15) == 0, "gd_adaln_modulate: x, mod and out must be 16-byte aligned");
    const size_t ob = ((size_t)(M - 1) * ldo + D) * 4;
    GD_REQUIRE(rl_disjoint(out, ob, mod, ((size_t)(M - 1) * ldm + 3 * (size_t)D) * 4), "gd_adaln_modulate: out overlaps mod");
    GD_REQUIRE((out == x && ldo == ldx) || rl_disjoint(out, ob, x, ((size_t)(M - 1) * ldx + D) * 4), "gd_adaln_modulate: out overlaps x without being x itself");
    const dim3 grid(gd_cdiv(M, 4)), blk(256);
    hipStream_t s = (hipStream_t)stream;
    const int nv = (D + 255) / 256;
#define AM_CALL(NV) hipLaunchKernelGGL((adaln_modulate_kernel<NV>), grid, blk, 0, s, x, mod, out, M, D, ldx, ldm, ldo, eps)
    if (nv <= 1) AM_CALL(1);
    else if (nv <= 2) AM_CALL(2);
    else if (nv <= 4) AM_CALL(4);
    else if (nv <= 8) AM_CALL(8);
    else if (nv <= 16) AM_CALL(16);
    else AM_CALL(32);
#undef AM_CALL
    GD_LAUNCH_OK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------------
// One launch per refinement iteration (camera_head.py:140-152, head_act.py:12-58) and, on the last one, the pose decoding
// (vggt/utils/pose_enc.py:108-126, vggt/utils/rotation.py:14-44).  One lane per row.
__device__ __forceinline__ float pose_act(float v, int code) {
    switch (code) {
    case 1: return (v > 0.f ? 1.f : v < 0.f ? -1.f : 0.f) * expm1f(fabsf(v));      // inv_log: sign(y) * expm1(|y|)
    case 2: return expf(v);
    case 3: return fmaxf(v, 0.f);
    default: return v;
    }
}

__global__ __launch_bounds__(64) void pose_update_kernel(const float* delta, long ldd, float* raw, float* enc, float* extrinsic, float* intrinsic, int M,
                                                         int first, int trans_act, int quat_act, int fl_act, float half_h, float half_w) {
    const int m = blockIdx.x * 64 + threadIdx.x;
    if (m >= M) return;
    float r[9], e[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        const float d = delta[(long)m * ldd + c];
        r[c] = first ? d : raw[m * 12 + c] + d;
        raw[m * 12 + c] = r[c];
        e[c] = pose_act(r[c], c < 3 ? trans_act : c < 7 ? quat_act : fl_act);
        enc[m * 9 + c] = e[c];
    }
    if (first) { raw[m * 12 + 9] = 0.f; raw[m * 12 + 10] = 0.f; raw[m * 12 + 11] = 0.f; }
    if (!extrinsic) return;
    const float qi = e[3], qj = e[4], qk = e[5], qr = e[6];
    const float two_s = 2.0f / (qi * qi + qj * qj + qk * qk + qr * qr);
    float* E = extrinsic + m * 12;
    E[0] = 1.f - two_s * (qj * qj + qk * qk); E[1] = two_s * (qi * qj - qk * qr);       E[2] = two_s * (qi * qk + qj * qr);        E[3] = e[0];
    E[4] = two_s * (qi * qj + qk * qr);       E[5] = 1.f - two_s * (qi * qi + qk * qk); E[6] = two_s * (qj * qk - qi * qr);        E[7] = e[1];
    E[8] = two_s * (qi * qk - qj * qr);       E[9] = two_s * (qj * qk + qi * qr);       E[10] = 1.f - two_s * (qi * qi + qj * qj); E[11] = e[2];
    float* Kc = intrinsic + m * 9;
    // a field of view of exactly 0 (relu of a negative value): tan(0) = 0 and half / 0 = +inf, as the reference's division gives
    Kc[0] = half_w / tanf(e[8] * 0.5f); Kc[1] = 0.f;                        Kc[2] = half_w;
    Kc[3] = 0.f;                        Kc[4] = half_h / tanf(e[7] * 0.5f); Kc[5] = half_h;
    Kc[6] = 0.f;                        Kc[7] = 0.f;                        Kc[8] = 1.f;
}

extern "C" int gd_pose_update(const float* delta, long ldd, float* raw, float* enc, float* extrinsic, float* intrinsic, int M, int first, int trans_act,
                              int quat_act, int fl_act, int H, int W, void* stream) {
    GD_REQUIRE(M >= 1 && M <= (1 << 20), "gd_pose_update: M = %d must be in [1, 2^20]", M);
    GD_REQUIRE(ldd >= 9, "gd_pose_update: ldd = %ld is below the 9 columns of delta", ldd);
    const int acts[3] = {trans_act, quat_act, fl_act};
    static const char* names[3] = {"trans_act", "quat_act", "fl_act"};
    for (int n = 0; n < 3; ++n)
        GD_REQUIRE(acts[n] >= 0 && acts[n] <= 3, "gd_pose_update: %s = %d: 0 linear, 1 inv_log, 2 exp, 3 relu", names[n], acts[n]);
    GD_REQUIRE(delta && raw && enc, "gd_pose_update: delta, raw and enc are required");
    GD_REQUIRE((((uintptr_t)delta | (uintptr_t)raw | (uintptr_t)enc | (uintptr_t)extrinsic | (uintptr_t)intrinsic) & 3) == 0,
               "gd_pose_update: every pointer must be 4-byte aligned");
    GD_REQUIRE((extrinsic == nullptr) == (intrinsic == nullptr), "gd_pose_update: pass both extrinsic and intrinsic or neither");
    GD_REQUIRE(!extrinsic || (H >= 1 && W >= 1), "gd_pose_update: the matrices need the image size (H = %d, W = %d)", H, W);
    hipLaunchKernelGGL(pose_update_kernel, dim3(gd_cdiv(M, 64)), dim3(64), 0, (hipStream_t)stream, delta, ldd, raw, enc, extrinsic, intrinsic, M, first,
                       trans_act, quat_act, fl_act, 0.5f * (float)H, 0.5f * (float)W);
    GD_LAUNCH_OK();
    return 0;
}
