// Per-head q/k LayerNorm + 2-D RoPE of the VGGT teacher's attention (vggt/layers/attention.py:58-65: q, k = q_norm(q), k_norm(k);
// q, k = rope(q, pos), rope(k, pos)), in place on the packed QKV-GEMM output qkv[B*N, 3*H*64] that gd_attention_fwd reads
// (q | k | v, heads inner).  v is never touched.  Optionally the results also leave as q_out / k_out [B, H, N, 64], the layout
// gd_cross_view_attn takes.
//     y = (x - mean_64) * rsqrt(var_64 + eps) * gamma + beta                       (fp32 statistics over the head's 64 channels)
//     quarters [u_Y, v_Y, u_X, v_X] of 16: theta = pos[axis] / base^(i/16);  u' = u cos - v sin;  v' = v cos + u sin   (gd_rope_2d)
// Memory-bound: a read and a write of two thirds of qkv.  One wave per token; a lane owns 16 bytes (CPL = 4 f32 / 8 bf16 channels) of a
// head, so LPH = 64 / CPL lanes cover a head and one wave-wide access covers 64 / LPH heads of the token's contiguous q | k columns.  The
// statistics are DPP sums over the LPH lanes, the rotation partner (16 channels away) sits LPH / 4 lanes away.  A token's 32 (cos, sin)
// pairs do not depend on the head: lanes 0..31 evaluate one pair each per token and every lane picks its CPL pairs up cross-lane, instead
// of CPL sincosf per lane.  No LDS.
#include "gd_common.h"

template <typename T> struct QkVec;
template <> struct QkVec<float> {
    static constexpr int CPL = 4;
    typedef f32x4 V;
    static __device__ __forceinline__ float get(const V& v, int j) { return v[j]; }
    static __device__ __forceinline__ void set(V& v, int j, float x) { v[j] = x; }
    // sum over the 16 lanes of a head
    static __device__ __forceinline__ float head_sum(float v) { return row16_sum(v); }
};
template <> struct QkVec<bf16> {
    static constexpr int CPL = 8;
    typedef bf16x8 V;
    static __device__ __forceinline__ float get(const V& v, int j) { return (float)v[j]; }
    static __device__ __forceinline__ void set(V& v, int j, float x) { v[j] = (bf16)x; }
    // sum over the 8 lanes of a head (half a DPP row)
    static __device__ __forceinline__ float head_sum(float v) {
        v += dpp_f32<0xB1, 0xF>(v);    // quad_perm [1,0,3,2]
        v += dpp_f32<0x4E, 0xF>(v);    // quad_perm [2,3,0,1]
        v += dpp_f32<0x141, 0xF>(v);   // row_half_mirror: the other quad of the 8
        return v;
    }
};

template <typename T, bool NORM>
__global__ __launch_bounds__(256) void qk_norm_rope_kernel(T* qkv, const long* pos, const float* gq, const float* bq, const float* gk,
                                                           const float* bk, T* q_out, T* k_out, int BN, int N, int H, float eps,
                                                           float base) {
    typedef QkVec<T> Q;
    constexpr int CPL = Q::CPL, LPH = 64 / CPL, HPW = 64 / LPH;     // channels per lane, lanes per head, heads per wave-wide access
    const int lane = threadIdx.x & 63;
    const int slot = lane % LPH, sub = lane / LPH, c0 = slot * CPL;      // this lane's channels [c0, c0 + CPL) of head (h0 + sub)
    const bool is_v = (c0 >> 4) & 1;                                      // v quarter: partner = the u quarter LPH / 4 lanes below
    const int pair0 = ((c0 >> 5) << 4) + (c0 & 15);                       // (axis, i) pair of channel c0 -> producer lane axis * 16 + i
    // producer role (lanes 0..31 do the work, 32..63 mirror them): pair p = lane & 31 -> axis p >> 4, frequency index p & 15
    const int p_axis = (lane >> 4) & 1;
    const float inv_freq = 1.0f / powf(base, (float)(lane & 15) / 16.0f);
    float g_q[CPL], b_q[CPL], g_k[CPL], b_k[CPL];
    if (NORM) {
#pragma unroll
        for (int j = 0; j < CPL; ++j) { g_q[j] = gq[c0 + j]; b_q[j] = bq[c0 + j]; g_k[j] = gk[c0 + j]; b_k[j] = bk[c0 + j]; }
    }
    const long ld = 3L * H * 64;
    const int nwaves = gridDim.x * 4;
    for (int tok = blockIdx.x * 4 + (threadIdx.x >> 6); tok < BN; tok += nwaves) {       // wave-uniform
        float sn, cs;
        sincosf((float)pos[(long)tok * 2 + p_axis] * inv_freq, &sn, &cs);
        float cj[CPL], sj[CPL];
#pragma unroll
        for (int j = 0; j < CPL; ++j) { cj[j] = __shfl(cs, pair0 + j, 64); sj[j] = __shfl(sn, pair0 + j, 64); }
        T* row = qkv + (long)tok * ld;
        const int b = tok / N, n = tok - b * N;
        for (int h0 = 0; h0 < 2 * H; h0 += HPW) {                 // the q | k columns are 2H consecutive heads of 64
            const int hh = h0 + sub;
            const bool live = hh < 2 * H;                          // whole heads (LPH lanes) are live or not: the cross-lane steps stay inside a head
            const bool isk = hh >= H;
            typename Q::V raw = {};
            float x[CPL];
            if (live) raw = *(const typename Q::V*)(row + (long)hh * 64 + c0);
#pragma unroll
            for (int j = 0; j < CPL; ++j) x[j] = live ? Q::get(raw, j) : 0.f;
            if (NORM) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < CPL; ++j) s += x[j];
                const float mu = Q::head_sum(s) * (1.0f / 64.0f);
                float q2 = 0.f;
#pragma unroll
                for (int j = 0; j < CPL; ++j) { x[j] -= mu; q2 += x[j] * x[j]; }
                const float rs = rsqrtf(Q::head_sum(q2) * (1.0f / 64.0f) + eps);
#pragma unroll
                for (int j = 0; j < CPL; ++j) x[j] = x[j] * rs * (isk ? g_k[j] : g_q[j]) + (isk ? b_k[j] : b_q[j]);
            }
            typename Q::V o;
#pragma unroll
            for (int j = 0; j < CPL; ++j) {
                const float other = __shfl_xor(x[j], LPH / 4, 64);          // the channel 16 away: u for a v lane, v for a u lane
                Q::set(o, j, is_v ? x[j] * cj[j] + other * sj[j] : x[j] * cj[j] - other * sj[j]);
            }
            if (live) {
                *(typename Q::V*)(row + (long)hh * 64 + c0) = o;
                T* dst = isk ? k_out : q_out;
                if (dst) *(typename Q::V*)(dst + (((long)b * H + (isk ? hh - H : hh)) * N + n) * 64 + c0) = o;
            }
        }
    }
}

extern "C" int gd_qk_norm_rope(void* qkv, const long* positions, const float* gamma_q, const float* beta_q, const float* gamma_k,
                               const float* beta_k, void* q_out, void* k_out, int B, int N, int H, int head_dim, float eps, float base,
                               int dtype, void* stream) {
    GD_REQUIRE(B > 0 && N > 0 && H > 0, "gd_qk_norm_rope: bad shape B=%d N=%d H=%d", B, N, H);
    GD_REQUIRE(head_dim == 64, "gd_qk_norm_rope: head_dim must be 64 (got %d)", head_dim);
    GD_REQUIRE((long)B * N < (1L << 31), "gd_qk_norm_rope: B * N must stay below 2^31 tokens");
    GD_REQUIRE(dtype == GD_F32 || dtype == GD_BF16, "gd_qk_norm_rope: bad dtype %d", dtype);
    GD_REQUIRE(qkv && positions, "gd_qk_norm_rope: qkv and positions must not be null");
    GD_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)q_out & 15) == 0 && ((uintptr_t)k_out & 15) == 0,
               "gd_qk_norm_rope: qkv, q_out and k_out must be 16-byte aligned");
    GD_REQUIRE((q_out == nullptr) == (k_out == nullptr), "gd_qk_norm_rope: pass both q_out and k_out or neither");
    const bool norm = gamma_q != nullptr;
    GD_REQUIRE((beta_q != nullptr) == norm && (gamma_k != nullptr) == norm && (beta_k != nullptr) == norm,
               "gd_qk_norm_rope: pass all four of gamma_q, beta_q, gamma_k, beta_k, or none (no normalisation)");
    GD_REQUIRE(base > 0.f && eps >= 0.f, "gd_qk_norm_rope: base must be positive and eps non-negative");
    const int BN = B * N, blocks = gd_cdiv(BN, 4);
    dim3 grid(blocks < 2048 ? blocks : 2048), blk(256);
    hipStream_t s = (hipStream_t)stream;
#define GD_QK_LAUNCH(T, NORM)                                                                                                          \
    hipLaunchKernelGGL((qk_norm_rope_kernel<T, NORM>), grid, blk, 0, s, (T*)qkv, positions, gamma_q, beta_q, gamma_k, beta_k, (T*)q_out, \
                       (T*)k_out, BN, N, H, eps, base)
    if (dtype == GD_BF16) { if (norm) GD_QK_LAUNCH(bf16, true); else GD_QK_LAUNCH(bf16, false); }
    else { if (norm) GD_QK_LAUNCH(float, true); else GD_QK_LAUNCH(float, false); }
#undef GD_QK_LAUNCH
    GD_LAUNCH_OK();
    return 0;
}
