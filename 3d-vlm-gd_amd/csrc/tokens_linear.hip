// gd_tokens_linear: y[M, N] = epilogue(x[M, K] . w[N, K]^T) in exact fp32 for token counts between gd_rows_linear (M <= 8, weight streaming) and
// gd_gemm_nt's 128 x 128 tiles: tens to a couple of thousand rows, hundreds of columns — the VGGT tracker's update transformer
// (teacher_tracker.FusedUpdateFormer(linear="tokens"): M = 728 / 600 / 128, N = 132 .. 1536, K = 384 / 388 / 1536), where a 128 x 128 tile leaves
// 3 to 72 workgroups on 256 compute units and every wave walks all of K for a 64 x 64 output.
//
//   * a workgroup of TL_WAVES = 4 waves owns ONE output tile of TM x 32 (TM = 32, or 64 once that still fills the device);
//   * the four waves split K: wave p takes the 16-k steps p, p + 4, p + 8, ...  In a step lane l loads the 16 bytes k = 16 s + 4 (l >> 4) .. + 3 of
//     row (l & 15) of each 16-row block of x and of w straight from global memory into VGPRs, TL_PF_* steps ahead of their use; MFMA number e of the
//     step's four v_mfma_f32_16x16x4_f32 contracts element e of both fragments (the same k permutation on both operands leaves the sum unchanged),
//     so no operand passes through LDS;
//   * the four partial tiles meet in LDS and are added in the fixed order (p0 + p1) + p2 + p3; then all 256 lanes apply the epilogue to 16-byte
//     pieces of the tile's rows: + bias, exact GELU, + residual, + y (accumulate) — gd_gemm_nt's order (gemm.hip) — and store them.
// The summation order of an output element depends on K alone: not on M, N, the tile height, the grid, the element's place in its tile or the row
// strides.  No split across workgroups, no atomics, no workspace.  A K tail (K % 16 != 0) contributes exact zeros from lane groups whose piece would
// start at or beyond K; they read the piece at k = 0 of their row instead and discard it.  Rows >= M and columns >= N of a partial tile load row M - 1 / column N - 1 again and store nothing.
#include "gd_common.h"

#define TL_WAVES 4
#define TL_KSTEP 16         // k per step of one wave: 4 lane groups x one 16-byte piece
#define TL_TN 32            // tile width
#define TL_PF_LOW 3         // steps whose operand loads are in flight ahead of the MFMAs: 32-row tiles (a step is 16 MFMAs, 512 cycles)
#define TL_PF_TALL 2        // 64-row tiles (32 MFMAs, 1024 cycles)
#define TL_TALL_MIN_WGS 512 // TM = 64 is taken when the grid of 64 x 32 tiles still has this many workgroups (two per compute unit of an MI355X)

struct TlArgs {
    const float *x, *w;
    float* y;
    const float *bias, *residual;
    int M, N, K, tiles_n, nwg;
    long ldx, ldw, ldy, ldr;
    int gelu, accumulate;
};

template <int TI, int PF> __global__ __launch_bounds__(64 * TL_WAVES) void tokens_linear_kernel(TlArgs a) {
    constexpr int TJ = TL_TN / 16, TM = 16 * TI, LDP = TL_TN + 4;          // LDP: 144-byte rows, the four lane groups of a store land on four bank quarters
    __shared__ __attribute__((aligned(16))) float part[TL_WAVES][TM * LDP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    const int wg = xcd_remap(blockIdx.x, a.nwg);
    const int tm = wg / a.tiles_n, tn = wg - tm * a.tiles_n;
    const int K = a.K, nsteps = (K + TL_KSTEP - 1) / TL_KSTEP;
    const float* xr[TI];
    const float* wr[TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i) xr[i] = a.x + (long)min(tm * TM + 16 * i + c, a.M - 1) * a.ldx;
#pragma unroll
    for (int j = 0; j < TJ; ++j) wr[j] = a.w + (long)min(tn * TL_TN + 16 * j + c, a.N - 1) * a.ldw;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = zero;

    // the pieces of step s: k = 16 s + 4 g .. + 3, all four below K or none (K % 4 == 0).  A lane group whose piece would start at or beyond K
    // (the K tail, and the steps a wave prefetches beyond its last) loads the piece at k = 0 instead — K >= 4: inside the row — and the step that
    // consumes it replaces it by zeros: no branch around a load and no use of a loaded value before its step, so the loads of the steps ahead stay
    // in flight across the MFMAs
    auto load = [&](int s, f32x4 (&fa)[TI], f32x4 (&fb)[TJ]) {
        const int k = s * TL_KSTEP + 4 * g;
        int ko = k < K ? k : 0;
        asm volatile("" : "+v"(ko));          // opaque to the optimiser, which otherwise moves every load down to its use one pass of the loop later
#pragma unroll
        for (int i = 0; i < TI; ++i) fa[i] = *(const f32x4*)(xr[i] + ko);
#pragma unroll
        for (int j = 0; j < TJ; ++j) fb[j] = *(const f32x4*)(wr[j] + ko);
    };
    f32x4 fa[PF][TI], fb[PF][TJ];
#pragma unroll
    for (int u = 0; u < PF; ++u) load(wave + TL_WAVES * u, fa[u], fb[u]);
    for (int s = wave; s < nsteps; s += TL_WAVES * PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            {   // no branch on s + TL_WAVES * u < nsteps: a step beyond the wave's last multiplies zeros (exact), and the loop body stays one
                // block whose waits count the loads in flight
                const bool live = (s + TL_WAVES * u) * TL_KSTEP + 4 * g < K;
                f32x4 ca[TI], cb[TJ];
#pragma unroll
                for (int i = 0; i < TI; ++i) ca[i] = live ? fa[u][i] : zero;
#pragma unroll
                for (int j = 0; j < TJ; ++j) cb[j] = live ? fb[u][j] : zero;
                load(s + TL_WAVES * (u + PF), fa[u], fb[u]);
                __builtin_amdgcn_sched_barrier(0);                          // the loads are issued before this step's MFMAs, not after them
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int i = 0; i < TI; ++i)
#pragma unroll
                        for (int j = 0; j < TJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ca[i][e], cb[j][e], acc[i][j], 0, 0, 0);
            }
        }
    }
    // ---- the four partial tiles: lane l holds rows 4 g + r, column c of every 16 x 16 block
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) part[wave][(16 * i + 4 * g + r) * LDP + 16 * j + c] = acc[i][j][r];
    __syncthreads();
    // ---- (p0 + p1) + p2 + p3, the epilogue and the store: one 16-byte piece of a row per lane and pass
    for (int e = threadIdx.x; e < TM * (TL_TN / 4); e += 64 * TL_WAVES) {
        const int row = e / (TL_TN / 4), c4 = (e % (TL_TN / 4)) * 4;
        const int m = tm * TM + row, n = tn * TL_TN + c4;
        if (m >= a.M || n >= a.N) continue;
        const f32x4 p0 = *(const f32x4*)&part[0][row * LDP + c4], p1 = *(const f32x4*)&part[1][row * LDP + c4];
        const f32x4 p2 = *(const f32x4*)&part[2][row * LDP + c4], p3 = *(const f32x4*)&part[3][row * LDP + c4];
        f32x4 v = ((p0 + p1) + p2) + p3;
        float* yr = a.y + (long)m * a.ldy + n;
        const float* rr = a.residual ? a.residual + (long)m * a.ldr + n : nullptr;
        if (n + 4 <= a.N) {
            if (a.bias) v += *(const f32x4*)(a.bias + n);
            if (a.gelu) { v[0] = gelu_f(v[0]); v[1] = gelu_f(v[1]); v[2] = gelu_f(v[2]); v[3] = gelu_f(v[3]); }
            if (rr) v += *(const f32x4*)rr;
            if (a.accumulate) v += *(const f32x4*)yr;
            *(f32x4*)yr = v;
        } else {                                                            // the last piece of an N that is no multiple of 4: element by element
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (n + q < a.N) {
                    float t = v[q];
                    if (a.bias) t += a.bias[n + q];
                    if (a.gelu) t = gelu_f(t);
                    if (rr) t += rr[q];
                    if (a.accumulate) t += yr[q];
                    yr[q] = t;
                }
            }
        }
    }
}

static bool tl_disjoint(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 + na <= b0 || b0 + nb <= a0;
}

extern "C" int gd_tokens_linear(const float* x, const float* w, float* y, int M, int N, int K, long ldx, long ldw, long ldy, const float* bias, int gelu,
                                const float* residual, long ldr, int accumulate, void* stream) {
    GD_REQUIRE(x, "gd_tokens_linear: x is null");
    GD_REQUIRE(w, "gd_tokens_linear: w is null");
    GD_REQUIRE(y, "gd_tokens_linear: y is null");
    GD_REQUIRE(M >= 1 && M <= (1 << 24), "gd_tokens_linear: M = %d must be in [1, 2^24]", M);
    GD_REQUIRE(N >= 1 && N <= (1 << 24), "gd_tokens_linear: N = %d must be in [1, 2^24]", N);
    GD_REQUIRE(K >= 4 && K % 4 == 0, "gd_tokens_linear: K = %d must be a positive multiple of 4", K);
    GD_REQUIRE(ldx >= K && ldx % 4 == 0, "gd_tokens_linear: ldx = %ld must be a multiple of 4 and >= K = %d", ldx, K);
    GD_REQUIRE(ldw >= K && ldw % 4 == 0, "gd_tokens_linear: ldw = %ld must be a multiple of 4 and >= K = %d", ldw, K);
    GD_REQUIRE(ldy >= N && ldy % 4 == 0, "gd_tokens_linear: ldy = %ld must be a multiple of 4 and >= N = %d", ldy, N);
    GD_REQUIRE(!residual || (ldr >= N && ldr % 4 == 0), "gd_tokens_linear: ldr = %ld must be a multiple of 4 and >= N = %d", ldr, N);
    GD_REQUIRE((uintptr_t)x % 16 == 0, "gd_tokens_linear: x %p must be 16-byte aligned", (const void*)x);
    GD_REQUIRE((uintptr_t)w % 16 == 0, "gd_tokens_linear: w %p must be 16-byte aligned", (const void*)w);
    GD_REQUIRE((uintptr_t)y % 16 == 0, "gd_tokens_linear: y %p must be 16-byte aligned", (void*)y);
    GD_REQUIRE((uintptr_t)bias % 16 == 0, "gd_tokens_linear: bias %p must be 16-byte aligned", (const void*)bias);
    GD_REQUIRE((uintptr_t)residual % 16 == 0, "gd_tokens_linear: residual %p must be 16-byte aligned", (const void*)residual);
    GD_REQUIRE(gelu == 0 || gelu == 1, "gd_tokens_linear: gelu %d: 0 (none) or 1 (exact GELU)", gelu);
    GD_REQUIRE(accumulate == 0 || accumulate == 1, "gd_tokens_linear: accumulate %d: 0 or 1", accumulate);
    const size_t ybytes = ((size_t)(M - 1) * ldy + N) * 4, xbytes = ((size_t)(M - 1) * ldx + K) * 4, wbytes = ((size_t)(N - 1) * ldw + K) * 4;
    GD_REQUIRE(tl_disjoint(y, ybytes, x, xbytes), "gd_tokens_linear: y [%p, +%zu) overlaps x [%p, +%zu)", (void*)y, ybytes, (const void*)x, xbytes);
    GD_REQUIRE(tl_disjoint(y, ybytes, w, wbytes), "gd_tokens_linear: y [%p, +%zu) overlaps w [%p, +%zu)", (void*)y, ybytes, (const void*)w, wbytes);
    if (residual) {
        // in place on the token stream: a piece is read and written by one lane.  Any other intersection would be a race.
        GD_REQUIRE((residual == y && ldr == ldy) || tl_disjoint(y, ybytes, residual, ((size_t)(M - 1) * ldr + N) * 4),
                   "gd_tokens_linear: y [%p, ld %ld] overlaps residual [%p, ld %ld] without being the same pointer and stride", (void*)y, ldy,
                   (const void*)residual, ldr);
    }
    TlArgs a;
    a.x = x; a.w = w; a.y = y; a.bias = bias; a.residual = residual;
    a.M = M; a.N = N; a.K = K; a.ldx = ldx; a.ldw = ldw; a.ldy = ldy; a.ldr = ldr; a.gelu = gelu; a.accumulate = accumulate;
    a.tiles_n = gd_cdiv(N, TL_TN);
    const long tall = (long)gd_cdiv(M, 64) * a.tiles_n, low = (long)gd_cdiv(M, 32) * a.tiles_n;
    GD_REQUIRE(low < (1L << 31), "gd_tokens_linear: M = %d x N = %d is %ld tiles, beyond the grid", M, N, low);
    // every offset in the kernel is 64-bit
    if (tall >= TL_TALL_MIN_WGS) {
        a.nwg = (int)tall;
        hipLaunchKernelGGL((tokens_linear_kernel<4, TL_PF_TALL>), dim3((unsigned)tall), dim3(64 * TL_WAVES), 0, (hipStream_t)stream, a);
    } else {
        a.nwg = (int)low;
        hipLaunchKernelGGL((tokens_linear_kernel<2, TL_PF_LOW>), dim3((unsigned)low), dim3(64 * TL_WAVES), 0, (hipStream_t)stream, a);
    }
    GD_LAUNCH_OK();
    return 0;
}
