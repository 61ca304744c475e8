// Multi-head attention for SHORT sequences of any small head dimension, exact fp32, addressed by strides: the VGGT tracker's update
// transformer (vggt/heads/track_modules/modules.py:170-218 AttnBlock / CrossAttnBlock on torch.nn.MultiheadAttention, between its input
// and output projections).  Its sequences are 2 rows (time stage), 64 and 300 rows (space stage), the head dimension is 48, and the
// space stage's tokens lie S * D apart in memory; gd_attention_fwd / gd_cross_attention_fwd (head dimension 64, 64-key LDS tiles, one
// batch stride) serve none of that.
//
// This is a latency kernel: the whole transformer's attention is ~0.1 GFLOP per call, so it is built for few instructions per launch
// and many waves in flight, on plain fmaf (exact f32, the rounding model an f32 MFMA would have).
//   * A TEAM of 16 lanes owns one query row of one (sequence, head); lane t of the team holds q[4t .. 4t+3] (pre-multiplied by
//     scale * log2 e) and accumulates output columns 4t .. 4t+3; lanes with 4t >= head_dim idle (they load nothing).
//   * A score is four fmaf per lane and one DPP row sum (row16_sum), k and v come straight from global / L2 with 16-byte loads:
//     no LDS, no barrier, no atomics.  Keys are walked in tiles of TILE with an online softmax, ONE rescale per tile.
//   * Short rows (Nk <= 8; the time stage): the four teams of a wave take four query rows — rows run (sequence, head, query), so a
//     wave holds several (sequence, head) items and the 2 x 2 problems of the time stage cost half a wave each; TILE = 2.
//   * Longer rows: the four teams of a wave split the keys of ONE query row in chunks of 8 and merge their (max, sum, acc) with two
//     shuffles, in a fixed order: bit-identical run to run.  64 queries x 300 keys then is 1024 waves of 75 keys, not 256 of 300.
#include "gd_common.h"

#define SA_MAX_HD 64

struct SaArgs {
    const float *q, *k, *v;
    float* o;
    int G1, Nq, Nk, H, hd;
    long ldq, ldk, ldv, ldo, sq0, sq1, sk0, sk1, sv0, sv1, so0, so1;
    float qmul;          // scale * log2(e)
    long rows;           // G0 * G1 * H * Nq
};

template <int KS, int TILE> __global__ __launch_bounds__(256) void sa_fwd_kernel(SaArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, team = lane >> 4, t = lane & 15;
    const long item = (long)blockIdx.x * 4 + wave;
    const long row = KS == 1 ? item * 4 + team : item;
    if (row >= a.rows) return;                                  // whole teams leave (KS == 1) or whole waves: the DPP rows stay complete
    const int i = (int)(row % a.Nq);
    const long gh = row / a.Nq;
    const int h = (int)(gh % a.H);
    const long g = gh / a.H, g0 = g / a.G1, g1 = g - g0 * a.G1;
    const bool active = 4 * t < a.hd;
    const long col = (long)h * a.hd + 4 * t;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 qs = zero;
    if (active) qs = *(const f32x4*)(a.q + g0 * a.sq0 + g1 * a.sq1 + (long)i * a.ldq + col) * a.qmul;
    const float* kb = a.k + g0 * a.sk0 + g1 * a.sk1 + col;
    const float* vb = a.v + g0 * a.sv0 + g1 * a.sv1 + col;
    const int Nk = a.Nk;
    float m = -INFINITY, l = 0.f;
    f32x4 acc = zero;
    for (int j0 = KS == 1 ? 0 : team * TILE; j0 < Nk; j0 += KS * TILE) {
        f32x4 kk[TILE], vv[TILE];
        float s[TILE];
#pragma unroll
        for (int u = 0; u < TILE; ++u) {                        // a key past the end reads the last row again and counts -inf
            const long jj = min(j0 + u, Nk - 1);
            kk[u] = active ? *(const f32x4*)(kb + jj * a.ldk) : zero;
            vv[u] = active ? *(const f32x4*)(vb + jj * a.ldv) : zero;
        }
        float tmax = -INFINITY;
#pragma unroll
        for (int u = 0; u < TILE; ++u) {
            float d = qs[0] * kk[u][0];
            d = fmaf(qs[1], kk[u][1], d);
            d = fmaf(qs[2], kk[u][2], d);
            d = fmaf(qs[3], kk[u][3], d);
            d = row16_sum(d);
            s[u] = j0 + u < Nk ? d : -INFINITY;
            tmax = fmaxf(tmax, s[u]);
        }
        const float mn = fmaxf(m, tmax);                        // finite: key j0 exists
        const float alpha = __builtin_amdgcn_exp2f(m - mn);     // 0 on the first tile (m = -inf)
        float psum = 0.f;
        f32x4 pv = zero;
#pragma unroll
        for (int u = 0; u < TILE; ++u) {
            const float p = __builtin_amdgcn_exp2f(s[u] - mn);
            psum += p;
            pv[0] = fmaf(p, vv[u][0], pv[0]);
            pv[1] = fmaf(p, vv[u][1], pv[1]);
            pv[2] = fmaf(p, vv[u][2], pv[2]);
            pv[3] = fmaf(p, vv[u][3], pv[3]);
        }
        l = fmaf(l, alpha, psum);
        acc = acc * alpha + pv;
        m = mn;
    }
    if (KS > 1) {
        // teams (0, 1) and (2, 3), then (0, 2): a team without keys (Nk < 8 * team + 1) carries m = -inf, l = 0 and weighs 0
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float mo = __shfl_xor(m, off, 64), lo = __shfl_xor(l, off, 64);
            f32x4 ao;
            ao[0] = __shfl_xor(acc[0], off, 64);
            ao[1] = __shfl_xor(acc[1], off, 64);
            ao[2] = __shfl_xor(acc[2], off, 64);
            ao[3] = __shfl_xor(acc[3], off, 64);
            const float mn = fmaxf(m, mo);
            const float wa = m == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m - mn);
            const float wb = mo == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mo - mn);
            l = fmaf(l, wa, lo * wb);
            acc = acc * wa + ao * wb;
            m = mn;
        }
        if (team != 0) return;
    }
    if (active) {
        f32x4 r;
        r[0] = acc[0] / l; r[1] = acc[1] / l; r[2] = acc[2] / l; r[3] = acc[3] / l;
        *(f32x4*)(a.o + g0 * a.so0 + g1 * a.so1 + (long)i * a.ldo + col) = r;
    }
}

// elements from the first to one past the last addressed cell of a tensor
static long sa_extent(int G0, int G1, int N, long s0, long s1, long ld, int width) {
    return (long)(G0 - 1) * s0 + (long)(G1 - 1) * s1 + (long)(N - 1) * ld + width;
}

extern "C" int gd_attention_small_fwd(const float* q, const float* k, const float* v, float* o, int G0, int G1, int Nq, int Nk, int H,
                                      int head_dim, long ldq, long ldk, long ldv, long ldo, long sq0, long sq1, long sk0, long sk1, long sv0,
                                      long sv1, long so0, long so1, float scale, void* stream) {
    GD_REQUIRE(head_dim >= 4 && head_dim <= SA_MAX_HD && head_dim % 4 == 0,
               "gd_attention_small_fwd: head_dim %d: a multiple of 4 from 4 to %d is served", head_dim, SA_MAX_HD);
    GD_REQUIRE(G0 >= 1 && G1 >= 1 && Nq >= 1 && Nk >= 1 && H >= 1, "gd_attention_small_fwd: need G0, G1, Nq, Nk, H >= 1 (G0=%d G1=%d Nq=%d Nk=%d H=%d)",
               G0, G1, Nq, Nk, H);
    const long lds[12] = {ldq, ldk, ldv, ldo, sq0, sq1, sk0, sk1, sv0, sv1, so0, so1};
    static const char* names[12] = {"ldq", "ldk", "ldv", "ldo", "sq0", "sq1", "sk0", "sk1", "sv0", "sv1", "so0", "so1"};
    for (int n = 0; n < 12; ++n)
        GD_REQUIRE(lds[n] >= 0 && lds[n] % 4 == 0, "gd_attention_small_fwd: stride %s = %ld must be a non-negative multiple of 4 elements", names[n], lds[n]);
    const int width = H * head_dim;
    GD_REQUIRE(ldq >= width && ldk >= width && ldv >= width && ldo >= width,
               "gd_attention_small_fwd: a row stride (ldq=%ld ldk=%ld ldv=%ld ldo=%ld) is below H * head_dim = %d", ldq, ldk, ldv, ldo, width);
    GD_REQUIRE(q && k && v && o, "gd_attention_small_fwd: q, k, v and o are required");
    GD_REQUIRE((((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)o) & 15) == 0, "gd_attention_small_fwd: q, k, v and o must be 16-byte aligned");
    // o against each input, by the range from the first to the last addressed cell (conservative: an o interleaved with an input is refused too)
    const float *ob = o, *oe = o + sa_extent(G0, G1, Nq, so0, so1, ldo, width);
    const float* ib[3] = {q, k, v};
    const float* ie[3] = {q + sa_extent(G0, G1, Nq, sq0, sq1, ldq, width), k + sa_extent(G0, G1, Nk, sk0, sk1, ldk, width),
                          v + sa_extent(G0, G1, Nk, sv0, sv1, ldv, width)};
    for (int n = 0; n < 3; ++n)
        GD_REQUIRE(oe <= ib[n] || ie[n] <= ob, "gd_attention_small_fwd: o overlaps %s", n == 0 ? "q" : n == 1 ? "k" : "v");
    SaArgs a;
    a.q = q; a.k = k; a.v = v; a.o = o;
    a.G1 = G1; a.Nq = Nq; a.Nk = Nk; a.H = H; a.hd = head_dim;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = ldo;
    a.sq0 = sq0; a.sq1 = sq1; a.sk0 = sk0; a.sk1 = sk1; a.sv0 = sv0; a.sv1 = sv1; a.so0 = so0; a.so1 = so1;
    a.qmul = scale * 1.4426950408889634f;
    a.rows = (long)G0 * G1 * H * Nq;
    const bool split = Nk > 8;
    const long waves = split ? a.rows : (a.rows + 3) / 4, blocks = (waves + 3) / 4;
    GD_REQUIRE(blocks < (1L << 31), "gd_attention_small_fwd: %ld query rows exceed the grid", a.rows);
    if (split)
        hipLaunchKernelGGL((sa_fwd_kernel<4, 8>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((sa_fwd_kernel<1, 2>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    GD_LAUNCH_OK();
    return 0;
}
