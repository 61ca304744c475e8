// Flash-style multi-head CROSS-attention forward (head_dim 64): the queries and the keys / values come from different token sets of
// different length.  The MASt3R teacher's decoder blocks (dust3r/croco/models/blocks.py:150-172, CrossAttention.forward between the
// projections and `proj`): o = softmax(q k^T * scale) v per (image, head).
//
// The form is attention.hip's register-staged forward kernel (attn_fwd_kernel), on the helpers of attn_common.h: the transposed formulation
// S^T = K Q^T, O^T += V^T P^T on 16x16 MFMA tiles, 4 waves x 32 queries per block, 64-key tiles staged one tile ahead through registers,
// softmax with a lagged reference point (the partial last key tile is a compile-time variant), row sums from the all-ones MFMA.  What differs:
// three bases and two row strides, queries bounded by Nq, key tiles / the tail mask / tile_load's nvalid bounded by Nk.
//   q  : [B, Nq, H*64], row stride ldq elements           kv : [B, Nk, 2, H, 64] (k | v, heads inner), row stride ldkv elements
//   o  : [B, Nq, H*64] contiguous                         lse: [B, H, Nq] natural log, may be null
#include "attn_common.h"

template <typename T>
__global__ __launch_bounds__(256, IsX3<T>::v ? 1 : 2) void cross_attn_fwd_kernel(const T* q, const T* kv, T* o, float* lse, int Nq, int Nk, int H,
                                                                                 long ldq_b, long ldkv_b, float scale) {
    constexpr int NF = AT<T>::NF, ROWB = AT<T>::ROWB;
    typedef typename Mma<T>::Frag Frag;
    __shared__ __attribute__((aligned(16))) char sK[64 * ROWB];
    __shared__ __attribute__((aligned(16))) char sV[TOp<T>::kNeedT ? 16 : 64 * ROWB];
    __shared__ __attribute__((aligned(16))) char sVt[TSZ(T)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    int xb_, h, b;
    attn_block_coords(xb_, h, b);
    const int q0 = xb_ * 128 + wave * 32;
    const char* qb = (const char*)q + (long)b * Nq * ldq_b + (long)h * HD * sizeof(T);
    const char* kb = (const char*)kv + (long)b * Nk * ldkv_b + (long)h * HD * sizeof(T);
    const char* vb = kb + (long)H * HD * sizeof(T);

    const float c2 = scale * 1.4426950408889634f;
    Frag qf[2][NF];       // q * scale * log2(e): the scores come out of the MFMA in the exp2 domain
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int qi = q0 + qt * 16 + c;
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            if (qi < Nq) qf[qt][u] = frag_scale<T>(load_nfrag<T>(qb + (long)qi * ldq_b, u, g), c2);
            else { Frag z = {}; qf[qt][u] = z; }
        }
    }
    f32x4 oacc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) oacc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m[2] = {0.f, 0.f};                                  // reference point, log2 units (see softmax_lagged)
    f32x4 negm[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 lacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};   // row sums (every row of the tile = the sum)
    const Frag ones = frag_ones<T>();

    TileRegs<T> rk, rv;
    tile_load<T>(rk, kb, ldkv_b, 0, Nk);
    tile_load<T>(rv, vb, ldkv_b, 0, Nk);
    // one 64-key tile; TAIL (compile-time) = the partial last tile, the only one whose keys need masking
    auto key_tile = [&](int k0, auto tail_tag) {
        constexpr bool tail = decltype(tail_tag)::value;
        __syncthreads();
        tile_store<T, true, false>(rk, sK, nullptr);
        tile_store<T, !TOp<T>::kNeedT, TOp<T>::kNeedT>(rv, sV, sVt);
        __syncthreads();
        if (k0 + 64 < Nk) {
            tile_load<T>(rk, kb, ldkv_b, k0 + 64, Nk);
            tile_load<T>(rv, vb, ldkv_b, k0 + 64, Nk);
        }
        f32x4 s[2][4];  // [qt][key tile]
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            Frag kf[NF];
#pragma unroll
            for (int u = 0; u < NF; ++u) kf[u] = lds_nfrag<T>(sK, kt * 16 + c, u, g);
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                f32x4 a = negm[qt];
#pragma unroll
                for (int u = 0; u < NF; ++u) a = Mma<T>::mma(kf[u], qf[qt][u], a);
                s[qt][kt] = a;
            }
        }
        softmax_lagged<tail>(s, m, negm, oacc, lacc, k0 == 0, k0, g, Nk);
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            Frag pf[2];
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                pf[qt] = acc_to_bfrag<T>(s[qt], u);
                lacc[qt] = Mma<T>::mma(ones, pf[qt], lacc[qt]);
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const Frag vf = TOp<T>::load(sV, sVt, dt, u, g, lane);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = Mma<T>::mma(vf, pf[qt], oacc[dt][qt]);
            }
        }
    };
    int k0 = 0;
    for (; k0 + 64 <= Nk; k0 += 64) key_tile(k0, std::false_type{});
    if (k0 < Nk) key_tile(k0, std::true_type{});
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int qi = q0 + qt * 16 + c;
        if (qi >= Nq) continue;
        const float lsum = lacc[qt][0];
        const float inv = 1.0f / lsum;
        T* orow = o + ((long)b * Nq + qi) * H * HD + h * HD;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4<T>(orow + dt * 16 + g * 4, oacc[dt][qt] * inv);
        if (lse != nullptr && g == 0) lse[((long)b * H + h) * Nq + qi] = (m[qt] + log2f(lsum)) * 0.6931471805599453f;   // natural log
    }
}

// ------------------------------------------------------------------------------------------ C ABI
// the element type of a dtype code, handed to `f` as a null pointer of that type (as attention.hip's attn_with_type)
template <typename F> static void cross_attn_with_type(int dtype, F f) {
    if (dtype == GD_BF16) f((bf16*)nullptr);
    else if (dtype == GD_F16) f((f16*)nullptr);
    else if (dtype == GD_F32X3) f((x3*)nullptr);
    else f((float*)nullptr);
}

extern "C" int gd_cross_attention_fwd(const void* q, const void* kv, void* o, float* lse, int B, int Nq, int Nk, int H, int head_dim,
                                      long ldq, long ldkv, float scale, int dtype, void* stream) {
    GD_REQUIRE(B > 0 && Nq > 0 && Nk > 0 && H > 0, "gd_cross_attention_fwd: bad shape B=%d Nq=%d Nk=%d H=%d", B, Nq, Nk, H);
    GD_REQUIRE(head_dim == HD, "gd_cross_attention_fwd: head_dim must be 64 (got %d)", head_dim);
    GD_REQUIRE(dtype == GD_F32 || dtype == GD_BF16 || dtype == GD_F32X3 || dtype == GD_F16, "gd_cross_attention_fwd: bad dtype %d", dtype);
    GD_REQUIRE(ldq >= (long)H * HD && ldkv >= (long)2 * H * HD,
               "gd_cross_attention_fwd: row strides too short: ldq=%ld (needs >= %d), ldkv=%ld (needs >= %d)", ldq, H * HD, ldkv, 2 * H * HD);
    const long esz = (dtype == GD_BF16 || dtype == GD_F16) ? 2 : 4;
    GD_REQUIRE(ldq * esz % 16 == 0 && ldkv * esz % 16 == 0, "gd_cross_attention_fwd: row strides must be multiples of 16 bytes: ldq=%ld ldkv=%ld", ldq,
               ldkv);
    GD_REQUIRE((long)Nq * ldq * 4 < (1L << 31), "gd_cross_attention_fwd: one image's q rows must span < 2^31 bytes (32-bit tile offsets): Nq=%d ldq=%ld",
               Nq, ldq);
    GD_REQUIRE((long)Nk * ldkv * 4 < (1L << 31),
               "gd_cross_attention_fwd: one image's kv rows must span < 2^31 bytes (32-bit tile offsets): Nk=%d ldkv=%ld", Nk, ldkv);
    GD_REQUIRE(q != nullptr && kv != nullptr && o != nullptr && ((uintptr_t)q & 15) == 0 && ((uintptr_t)kv & 15) == 0 && ((uintptr_t)o & 15) == 0,
               "gd_cross_attention_fwd: q, kv, o must be non-null and 16-byte aligned");
    const dim3 grid(gd_cdiv(Nq, 128), H, B);
    cross_attn_with_type(dtype, [&](auto* t) {
        typedef std::remove_pointer_t<decltype(t)> T;
        hipLaunchKernelGGL(cross_attn_fwd_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, (const T*)q, (const T*)kv, (T*)o, lse, Nq, Nk, H,
                           ldq * (long)sizeof(T), ldkv * (long)sizeof(T), scale);
    });
    GD_LAUNCH_OK();
    return 0;
}
