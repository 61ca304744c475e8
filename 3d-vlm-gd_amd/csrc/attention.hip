// Flash-style multi-head self-attention for the student ViT (head_dim 64), forward and backward,
// on 16x16 MFMA tiles in a TRANSPOSED formulation (gfx950):
//
//   forward, per wave 32 queries:   S^T = K Q^T   (keys on C-rows, queries on C-columns = lanes)
//                                   O^T += V^T P^T
//   With queries on the lane axis the softmax statistics (m, l) and the rescale factor are per-lane
//   scalars, the row reductions are in-register plus two cross-lane-group shuffles, and the S^T
//   accumulator tiles are directly the B operand of the second product (k-slot permutation shared
//   with the transposed V tile) — P never goes through LDS.
//
//   backward = two kernels (deterministic, no atomics):
//     attn_bwd_dq  (query owner): recompute S^T, dP^T = V dO^T, dS^T = P^T o (dP^T - delta), dQ^T += K^T dS^T
//     attn_bwd_dkv (key owner)  : S = Q K^T, dP = dO V^T, dV^T += dO^T P, dK^T += Q^T dS
//
// Replaces F.scaled_dot_product_attention inside timm's Attention (restated from
// vggt/layers/attention.py:51-71): softmax((q*scale) k^T) v with scale = head_dim^-0.5.
// qkv is the packed [B, N, 3, H, 64] output of the QKV GEMM; o is [B, N, H*64]; lse is [B, H, N] (natural log).
#include "attn_common.h"

// ------------------------------------------------------------------------------------------ forward
template <typename T>
__global__ __launch_bounds__(256, 2) void attn_fwd_kernel(const T* qkv, T* o, float* lse, int N, int H, float scale) {
    constexpr int NF = AT<T>::NF, ROWB = AT<T>::ROWB;
    typedef typename Mma<T>::Frag Frag;
    __shared__ __attribute__((aligned(16))) char sK[64 * ROWB];
    __shared__ __attribute__((aligned(16))) char sV[TOp<T>::kNeedT ? 16 : 64 * ROWB];
    __shared__ __attribute__((aligned(16))) char sVt[TSZ(T)];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    int xb_, h, b;
    attn_block_coords(xb_, h, b);
    const int q0 = xb_ * 128 + wave * 32;
    const long ld_b = (long)3 * H * HD * sizeof(T);
    const char* base = (const char*)qkv + (long)b * N * ld_b;
    const char* qb = base + (long)(0 * H + h) * HD * sizeof(T);
    const char* kb = base + (long)(1 * H + h) * HD * sizeof(T);
    const char* vb = base + (long)(2 * H + h) * HD * sizeof(T);

    const float c2 = scale * 1.4426950408889634f;
    Frag qf[2][NF];       // q * scale * log2(e): the scores come out of the MFMA in the exp2 domain
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + c;
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            if (q < N) qf[qt][u] = frag_scale<T>(load_nfrag<T>(qb + (long)q * ld_b, u, g), c2);
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
    tile_load<T>(rk, kb, ld_b, 0, N);
    tile_load<T>(rv, vb, ld_b, 0, N);
    // one 64-key tile; TAIL (compile-time) = the partial last tile, the only one whose keys need masking — as a run-time
    // flag the mask was if-converted into 60 compare/select instructions in EVERY tile of a VALU-bound loop
    auto key_tile = [&](int k0, auto tail_tag) {
        constexpr bool tail = decltype(tail_tag)::value;
        __syncthreads();
        tile_store<T, true, false>(rk, sK, nullptr);
        tile_store<T, !TOp<T>::kNeedT, TOp<T>::kNeedT>(rv, sV, sVt);
        __syncthreads();
        if (k0 + 64 < N) {
            tile_load<T>(rk, kb, ld_b, k0 + 64, N);
            tile_load<T>(rv, vb, ld_b, k0 + 64, N);
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
        softmax_lagged<tail>(s, m, negm, oacc, lacc, k0 == 0, k0, g, N);
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
    for (; k0 + 64 <= N; k0 += 64) key_tile(k0, std::false_type{});
    if (k0 < N) key_tile(k0, std::true_type{});
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + c;
        if (q >= N) continue;
        const float lsum = lacc[qt][0];
        const float inv = 1.0f / lsum;
        T* orow = o + ((long)b * N + q) * H * HD + h * HD;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4<T>(orow + dt * 16 + g * 4, oacc[dt][qt] * inv);
        if (g == 0) lse[((long)b * H + h) * N + q] = (m[qt] + log2f(lsum)) * 0.6931471805599453f;   // natural log
    }
}

// ------------------------------------------------------------------------------------------ forward, bf16, LDS-DMA
// Same mathematics and register layout as attn_fwd_kernel, but K / V tiles travel global -> LDS by LDS-DMA
// (global_load_lds_dwordx4) into a THREE-slot ring, two tiles ahead, with no staging registers: at N = 1370 one tile of
// prefetch distance (~0.9 us) is shorter than a loaded memory round trip and 31 % of the wave cycles sat in s_waitcnt
// vmcnt.  Rows are 128 bytes unpadded (a DMA piece is 8 rows x 128 B, lane-linear in LDS); the 16-byte chunk index is
// XOR-swizzled with (row >> 1) & 7 on the SOURCE address, as in the GEMM, so the K fragment reads (ds_read_b128) and the
// V transpose reads (ds_read_b64_tr_b16) stay conflict-free.  All LDS reads are inline asm (a ds_read the compiler can see
// gets an `s_waitcnt vmcnt` to the most recent LDS-DMA in front of it); one counted vmcnt wait + one barrier per tile.
// Key rows past N are clamped to row N-1: their scores are masked in the (compile-time) tail tile, so p = 0 for them.
// Round 6: the tiles whose two-ahead prefetch is a full tile run in groups of THREE with the ring slot as a compile-time constant — every LDS read is
// base register + immediate (no per-tile address arithmetic on the vector ALU) and the slot / wait-kind / full-tile / rotation tests leave the loop:
// ~30 scalar instructions per tile instead of ~60 (the round-5 loop executed 1.40 scalar per MFMA, profiles/r05_pmc_attention_stall.json; the non-MFMA
// vector count per steady-state tile is what it was, ~80: 32 v_exp, 16 v_cvt_pk, 16 v_max3 + the threshold test, 4 64-bit address adds for the DMA —
// the compiler keeps the per-lane piece pointers as 64-bit pairs whatever the source says).  Bit-identical; 423.0 -> 416.6 us at 64 x 12 x 1370,
// 1016.8 -> 998.7 us at 8 x 12 x 6401, 57.58 -> 57.50 ms per step in one process (profiles/r06_probe_attn_tn.txt).  The tiles the groups do not
// cover (the last two full tiles, up to two more, the partial tail) run the generic loop below.
template <typename T>      // bf16 | f16
__global__ __launch_bounds__(256, 2) void attn_fwd_dma_kernel(const T* qkv, T* o, float* lse, int N, int H, float scale, int rot_on) {
    typedef typename Mma<T>::Frag Frag;
    constexpr int TILE = 64 * 128;                       // one K or V tile: 64 rows x 128 B
    __shared__ __attribute__((aligned(16))) char smem[6 * TILE];   // K slots 0..2 | V slots 0..2
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int xb_, h, b;
    attn_block_coords(xb_, h, b);
    const int q0 = xb_ * 128 + wave * 32;
    const long ld_b = (long)3 * H * HD * 2;
    const char* base = (const char*)qkv + (long)b * N * ld_b;
    const char* qb = base + (long)(0 * H + h) * HD * 2;
    const char* kb = base + (long)(1 * H + h) * HD * 2;
    const char* vb = base + (long)(2 * H + h) * HD * 2;

    const float c2 = scale * 1.4426950408889634f;
    Frag qf[2][2];        // q * scale * log2(e)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + c;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (q < N) qf[qt][u] = frag_scale<T>(load_nfrag<T>(qb + (long)q * ld_b, u, g), c2);
            else { Frag z = {}; qf[qt][u] = z; }
        }
    }
    // DMA: wave w moves pieces 2w, 2w+1 (8 rows each) of the K tile and of the V tile
    const int prow = lane >> 3, pchunk = lane & 7;
    // per-piece source pointers of tile 0 (loop-invariant); a full tile adds the scalar k0 * ld_b — the clamped form (one 64-bit
    // multiply per piece: 10 VALU instructions, two of them quarter-rate) is only needed for the partial last tile
    const char* kp[2];
    const char* vp_[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wave * 2 + i) * 8 + prow;
        const long off = (long)row * ld_b + ((pchunk ^ AT<T>::sw(row)) * 16);
        kp[i] = kb + off;
        vp_[i] = vb + off;
    }
    auto issue = [&](int k0, int slot) {
        if (k0 + 64 <= N) {
            const unsigned long t0 = (unsigned)k0 * (unsigned)ld_b;     // 32-bit scalar product (an image's qkv rows span < 2^31 bytes)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kp[i] + t0),
                                                 (__attribute__((address_space(3))) void*)(smem + slot * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vp_[i] + t0),
                                                 (__attribute__((address_space(3))) void*)(smem + (3 + slot) * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (wave * 2 + i) * 8 + prow;
            const long off = (long)min(k0 + row, N - 1) * ld_b + ((pchunk ^ AT<T>::sw(row)) * 16);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kb + off),
                                             (__attribute__((address_space(3))) void*)(smem + slot * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vb + off),
                                             (__attribute__((address_space(3))) void*)(smem + (3 + slot) * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
        }
    };
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)smem;
    // K fragment (kt, u): row kt*16 + c, logical chunk 4u + g
    const int swk = AT<T>::sw(c);
    const unsigned ka0 = c * 128 + ((0 + g) ^ swk) * 16, ka1 = c * 128 + ((4 + g) ^ swk) * 16;
    // V transpose fragment (dt, u): rows 32u + 4g + q (+16), logical chunk 2dt + (p>>1), 8-byte half p&1
    const int vq = c >> 2, vp = c & 3, swv = AT<T>::sw(4 * g + vq);
    unsigned va[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) va[dt] = (4 * g + vq) * 128 + (((2 * dt + (vp >> 1)) ^ swv) * 16) + 8 * (vp & 1);

    f32x4 oacc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) oacc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m[2] = {0.f, 0.f};                                  // reference point, log2 units (see softmax_lagged)
    f32x4 negm[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    f32x4 lacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    const Frag ones = frag_ones<T>();
    const int ntile = (N + 63) / 64, nfull = N / 64;
    // The x-blocks of an (image, head) start together on one XCD and sweep the same K / V tiles at the same pace: in
    // lockstep they all ask one L2 channel for the same lines at the same moment.  Softmax accumulation does not care about
    // the key order, so block xb starts at full tile (2 xb) mod nfull and wraps; the partial tail tile stays last (its
    // mask is the compile-time variant of the tile body).
    const int rot = (nfull > 0 && rot_on) ? (2 * xb_) % nfull : 0;
    auto pk0 = [&](int t) { return (t < nfull ? (t + rot >= nfull ? t + rot - nfull : t + rot) : t) * 64; };
    issue(pk0(0), 0);
    if (ntile > 1) issue(pk0(1), 1);
    int slot = 0;            // t % 3, kept as a running scalar (the modulo was strength-reduced into per-address VALU fix-ups)
    auto key_tile = [&](int t, auto tail_tag) {
        constexpr bool tail = decltype(tail_tag)::value;
        const int k0 = pk0(t);
        if (t + 1 < ntile) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // tile t landed; tile t+1 may still fly
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();            // everyone's pieces of tile t landed; everyone is done with tile t-1's slot
        asm volatile("" ::: "memory");
        if (t + 2 < ntile) issue(pk0(t + 2), slot == 0 ? 2 : slot - 1);
        if (q0 >= N) return;      // (lambda) a wave whose 32 queries are all past N only moves its DMA pieces
        const unsigned kbase = lds0 + slot * TILE, vbase = lds0 + (3 + slot) * TILE;
        f32x4 kr[4][2];
        ADS_R128(kr[0][0], kbase + ka0, 0);    ADS_R128(kr[0][1], kbase + ka1, 0);
        ADS_R128(kr[1][0], kbase + ka0, 2048); ADS_R128(kr[1][1], kbase + ka1, 2048);
        ADS_R128(kr[2][0], kbase + ka0, 4096); ADS_R128(kr[2][1], kbase + ka1, 4096);
        ADS_R128(kr[3][0], kbase + ka0, 6144); ADS_R128(kr[3][1], kbase + ka1, 6144);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kr[0][0]), "+v"(kr[0][1]), "+v"(kr[1][0]), "+v"(kr[1][1]), "+v"(kr[2][0]), "+v"(kr[2][1]),
                     "+v"(kr[3][0]), "+v"(kr[3][1]));
        f32x4 s[2][4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                f32x4 a = negm[qt];
#pragma unroll
                for (int u = 0; u < 2; ++u) a = Mma<T>::mma(__builtin_bit_cast(Frag, kr[kt][u]), qf[qt][u], a);
                s[qt][kt] = a;
            }
        // V fragments: issued now, consumed after the softmax
        a_u32x2 vr[4][2][2];   // [dt][u][row half]
#define ADS_V(dt)                                                                                   \
        ADS_TR64(vr[dt][0][0], vbase + va[dt], 0);    ADS_TR64(vr[dt][0][1], vbase + va[dt], 2048);     \
        ADS_TR64(vr[dt][1][0], vbase + va[dt], 4096); ADS_TR64(vr[dt][1][1], vbase + va[dt], 6144);
        ADS_V(0) ADS_V(1) ADS_V(2) ADS_V(3)
#undef ADS_V
        softmax_lagged<tail>(s, m, negm, oacc, lacc, t == 0, k0, g, N);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vr[0][0][0]), "+v"(vr[0][0][1]), "+v"(vr[0][1][0]), "+v"(vr[0][1][1]), "+v"(vr[1][0][0]),
                     "+v"(vr[1][0][1]), "+v"(vr[1][1][0]), "+v"(vr[1][1][1]), "+v"(vr[2][0][0]), "+v"(vr[2][0][1]), "+v"(vr[2][1][0]),
                     "+v"(vr[2][1][1]), "+v"(vr[3][0][0]), "+v"(vr[3][0][1]), "+v"(vr[3][1][0]), "+v"(vr[3][1][1]));
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            Frag pf[2];
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                pf[qt] = acc_to_bfrag<T>(s[qt], u);
                lacc[qt] = Mma<T>::mma(ones, pf[qt], lacc[qt]);
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                typedef __attribute__((ext_vector_type(4))) unsigned a_u32x4;
                const a_u32x4 z = {vr[dt][u][0][0], vr[dt][u][0][1], vr[dt][u][1][0], vr[dt][u][1][1]};
                const Frag vf = __builtin_bit_cast(Frag, z);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = Mma<T>::mma(vf, pf[qt], oacc[dt][qt]);
            }
        }
    };
    int t = 0;
    {
        // ---- steady state: tiles t with t + 2 < nfull, three at a time (slot = t % 3 is the compile-time S of each copy)
        const int nsteady = nfull > 2 ? (nfull - 2) / 3 * 3 : 0;
        const bool live = q0 < N;                // (a wave whose 32 queries are all past N only moves its DMA pieces)
        const unsigned voff[2] = {(unsigned)(kp[0] - kb), (unsigned)(kp[1] - kb)};      // this lane's byte offset inside a tile, per piece (< 64 rows x ld_b < 2^31)
        int kt2 = nsteady ? pk0(2) : 0;          // first key of the tile two ahead, kept as a running scalar (+64, wrapping at nfull * 64)
        const int kwrap = nfull * 64;
        auto step = [&](auto slot_c, bool first) __attribute__((always_inline)) {
            constexpr int S = decltype(slot_c)::value, S2 = (S + 2) % 3;
            asm volatile("s_waitcnt vmcnt(4)" ::: "memory");      // tile t landed; tile t + 1 may still fly
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            {
                const unsigned long t0 = (unsigned)kt2 * (unsigned)ld_b;
                const char* ks = kb + t0;        // scalar tile bases: the pieces go out as saddr + 32-bit voffset
                const char* vs = vb + t0;
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(ks + voff[i]),
                                                     (__attribute__((address_space(3))) void*)(smem + S2 * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vs + voff[i]),
                                                     (__attribute__((address_space(3))) void*)(smem + (3 + S2) * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
                }
                kt2 += 64;
                if (kt2 == kwrap) kt2 = 0;
            }
            if (!live) return;
            const unsigned ak0 = lds0 + ka0, ak1 = lds0 + ka1;
            f32x4 kr[4][2];
            ADS_R128(kr[0][0], ak0, S * TILE + 0);    ADS_R128(kr[0][1], ak1, S * TILE + 0);
            ADS_R128(kr[1][0], ak0, S * TILE + 2048); ADS_R128(kr[1][1], ak1, S * TILE + 2048);
            ADS_R128(kr[2][0], ak0, S * TILE + 4096); ADS_R128(kr[2][1], ak1, S * TILE + 4096);
            ADS_R128(kr[3][0], ak0, S * TILE + 6144); ADS_R128(kr[3][1], ak1, S * TILE + 6144);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kr[0][0]), "+v"(kr[0][1]), "+v"(kr[1][0]), "+v"(kr[1][1]), "+v"(kr[2][0]), "+v"(kr[2][1]),
                         "+v"(kr[3][0]), "+v"(kr[3][1]));
            f32x4 s[2][4];
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) {
                    f32x4 a = negm[qt];
#pragma unroll
                    for (int u = 0; u < 2; ++u) a = Mma<T>::mma(__builtin_bit_cast(Frag, kr[kt][u]), qf[qt][u], a);
                    s[qt][kt] = a;
                }
            a_u32x2 vr[4][2][2];   // [dt][u][row half]
#define ADS_VI(dt)                                                                                                                   \
            ADS_TR64(vr[dt][0][0], lds0 + va[dt], (3 + S) * TILE + 0);    ADS_TR64(vr[dt][0][1], lds0 + va[dt], (3 + S) * TILE + 2048);       \
            ADS_TR64(vr[dt][1][0], lds0 + va[dt], (3 + S) * TILE + 4096); ADS_TR64(vr[dt][1][1], lds0 + va[dt], (3 + S) * TILE + 6144);
            ADS_VI(0) ADS_VI(1) ADS_VI(2) ADS_VI(3)
#undef ADS_VI
            softmax_lagged<false>(s, m, negm, oacc, lacc, first, 0, g, N);
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vr[0][0][0]), "+v"(vr[0][0][1]), "+v"(vr[0][1][0]), "+v"(vr[0][1][1]), "+v"(vr[1][0][0]),
                         "+v"(vr[1][0][1]), "+v"(vr[1][1][0]), "+v"(vr[1][1][1]), "+v"(vr[2][0][0]), "+v"(vr[2][0][1]), "+v"(vr[2][1][0]),
                         "+v"(vr[2][1][1]), "+v"(vr[3][0][0]), "+v"(vr[3][0][1]), "+v"(vr[3][1][0]), "+v"(vr[3][1][1]));
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                Frag pf[2];
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) {
                    pf[qt] = acc_to_bfrag<T>(s[qt], u);
                    lacc[qt] = Mma<T>::mma(ones, pf[qt], lacc[qt]);
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    typedef __attribute__((ext_vector_type(4))) unsigned a_u32x4;
                    const a_u32x4 z = {vr[dt][u][0][0], vr[dt][u][0][1], vr[dt][u][1][0], vr[dt][u][1][1]};
                    const Frag vf = __builtin_bit_cast(Frag, z);
#pragma unroll
                    for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = Mma<T>::mma(vf, pf[qt], oacc[dt][qt]);
                }
            }
        };
        for (; t < nsteady; t += 3) {
            step(std::integral_constant<int, 0>{}, t == 0);
            step(std::integral_constant<int, 1>{}, false);
            step(std::integral_constant<int, 2>{}, false);
        }
        // (nsteady is a multiple of three: the generic tiles below start at slot 0 again)
    }
    for (; (t + 1) * 64 <= N; ++t) {
        key_tile(t, std::false_type{});
        slot = slot == 2 ? 0 : slot + 1;
    }
    if (t * 64 < N) key_tile(t, std::true_type{});
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + c;
        if (q >= N) continue;
        const float lsum = lacc[qt][0];
        const float inv = 1.0f / lsum;
        T* orow = o + ((long)b * N + q) * H * HD + h * HD;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4<T>(orow + dt * 16 + g * 4, oacc[dt][qt] * inv);
        if (g == 0) lse[((long)b * H + h) * N + q] = (m[qt] + log2f(lsum)) * 0.6931471805599453f;
    }
}

// ------------------------------------------------------------------------------------------ backward: dQ
template <typename T>
__global__ __launch_bounds__(256, IsX3<T>::v ? 1 : 2) void attn_bwd_dq_kernel(const T* qkv, const T* o, const T* dout, const float* lse,
                                                          float* delta, T* dqkv, int N, int H, float scale) {
    constexpr int NF = AT<T>::NF, ROWB = AT<T>::ROWB;
    typedef typename Mma<T>::Frag Frag;
    __shared__ __attribute__((aligned(16))) char sK[64 * ROWB];
    __shared__ __attribute__((aligned(16))) char sKt[TSZ(T)];
    __shared__ __attribute__((aligned(16))) char sV[64 * ROWB];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    int xb_, h, b;
    attn_block_coords(xb_, h, b);
    const int q0 = xb_ * 128 + wave * 32;
    const int npad = (N + 63) / 64 * 64;
    const long ld_b = (long)3 * H * HD * sizeof(T);
    const char* base = (const char*)qkv + (long)b * N * ld_b;
    const char* qb = base + (long)(0 * H + h) * HD * sizeof(T);
    const char* kb = base + (long)(1 * H + h) * HD * sizeof(T);
    const char* vb = base + (long)(2 * H + h) * HD * sizeof(T);
    const long ldo_b = (long)H * HD * sizeof(T);
    const char* dob = (const char*)dout + (long)b * N * ldo_b + (long)h * HD * sizeof(T);
    const char* ob = (const char*)o + (long)b * N * ldo_b + (long)h * HD * sizeof(T);

    // delta = rowsum(dO * O) is taken here, from the dO fragments this wave loads anyway (+ the matching O fragments), and
    // written for the dK/dV kernel that runs next on the stream — it used to be its own pass over O and dO.
    Frag qf[2][NF], dof[2][NF];
    float lq[2], dl[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + c;
        const bool ok = q < N;
        float dsum = 0.f;
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            Frag z = {};
            qf[qt][u] = ok ? frag_scale<T>(load_nfrag<T>(qb + (long)q * ld_b, u, g), scale * 1.4426950408889634f) : z;   // exp2 domain
            dof[qt][u] = ok ? load_nfrag<T>(dob + (long)q * ldo_b, u, g) : z;
            const Frag of_ = ok ? load_nfrag<T>(ob + (long)q * ldo_b, u, g) : z;
            dsum += frag_dot(dof[qt][u], of_);
        }
        dsum += __shfl_xor(dsum, 16, 64);      // the four lane groups g hold the four 16-byte pieces of each K-chunk
        dsum += __shfl_xor(dsum, 32, 64);
        lq[qt] = ok ? lse[((long)b * H + h) * N + q] * 1.4426950408889634f : 0.f;   // log2 units
        dl[qt] = dsum;
        // row constants for the dK/dV kernel, in the form its accumulators start from: ws[0] = -delta, ws[1] = -lse (log2 units), rows padded to whole
        // 64-query tiles — a pad query gets -lse = -1e30, i.e. p = exp2(s - 1e30) = 0 and dS = 0 whatever row its tile slot holds
        if (g == 0 && q < npad) {
            const long wi = ((long)b * H + h) * npad + q;
            delta[wi] = ok ? -dsum : 0.f;
            delta[(long)gridDim.z * H * npad + wi] = ok ? -lq[qt] : -1e30f;
        }
    }
    f32x4 dq[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) dq[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // row constants as the initial accumulators (the MFMA's C operand): S' = q k c2 - lse2 and dP' = dO v - delta leave the
    // chains ready, p = exp2(S') and dS = p * dP' — one v_exp and one multiply per score, no subtract / scale FMA
    f32x4 nlq[2], ndl[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        nlq[qt] = f32x4{-lq[qt], -lq[qt], -lq[qt], -lq[qt]};
        ndl[qt] = f32x4{-dl[qt], -dl[qt], -dl[qt], -dl[qt]};
    }

    // (key tiles in plain order: a per-block rotated order, which helps the forward kernel a little, measured 4 % SLOWER here —
    //  the blocks of an (image, head) trail each other through the L2 and the rotation takes that away)
    const int ntile = (N + 63) / 64;
    auto pk0 = [&](int t) { return t * 64; };
    TileRegs<T> rk, rv;
    TileSrc<T> ksrc, vsrc;
    tile_src_init<T>(ksrc, kb, ld_b, N);
    tile_src_init<T>(vsrc, vb, ld_b, N);
    tile_load<T>(rk, ksrc, pk0(0));
    tile_load<T>(rv, vsrc, pk0(0));
    // TAIL (compile-time): the partial last tile.  Keys >= N are staged as zero K / V rows, so their dS never reaches dQ through the product — but
    // their p = exp2(0 - lse2) is unbounded when the row's scores are all far below zero (lse2 << 0), and a 16-bit dS = p * dP' that overflows to
    // inf makes inf * 0 = NaN in the dQ product (fp16: 5 exponent bits; found by the all_negative case of test_attention_reference_point_moves).
    // Their dS is therefore set to zero, in the tail tile only.
    auto key_tile = [&](int t, auto tail_tag) {
        constexpr bool tail = decltype(tail_tag)::value;
        __syncthreads();
        tile_store<T, true, TOp<T>::kNeedT>(rk, sK, sKt);
        tile_store<T, true, false>(rv, sV, nullptr);
        __syncthreads();
        if (t + 1 < ntile) {
            tile_load<T>(rk, ksrc, pk0(t + 1));
            tile_load<T>(rv, vsrc, pk0(t + 1));
        }
        if (q0 >= N) return;   // a wave whose 32 queries are all past N only helps staging
        f32x4 ds[2][4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            Frag kf[NF], vf[NF];
#pragma unroll
            for (int u = 0; u < NF; ++u) {
                kf[u] = lds_nfrag<T>(sK, kt * 16 + c, u, g);
                vf[u] = lds_nfrag<T>(sV, kt * 16 + c, u, g);
            }
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) {
                f32x4 s = nlq[qt], dp = ndl[qt];
#pragma unroll
                for (int u = 0; u < NF; ++u) {
                    s = Mma<T>::mma(kf[u], qf[qt][u], s);
                    dp = Mma<T>::mma(vf[u], dof[qt][u], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    ds[qt][kt][r] = fast_exp2(s[r]) * dp[r];       // the 1/sqrt(d) factor is applied once, to dQ
                    if (tail && t * 64 + kt * 16 + g * 4 + r >= N) ds[qt][kt][r] = 0.f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            Frag df[2];
#pragma unroll
            for (int qt = 0; qt < 2; ++qt) df[qt] = acc_to_bfrag<T>(ds[qt], u);
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const Frag kf = TOp<T>::load(sK, sKt, dt, u, g, lane);
#pragma unroll
                for (int qt = 0; qt < 2; ++qt) dq[dt][qt] = Mma<T>::mma(kf, df[qt], dq[dt][qt]);
            }
        }
    };
    {
        int t = 0;
        for (; (t + 1) * 64 <= N; ++t) key_tile(t, std::false_type{});
        if (t * 64 < N) key_tile(t, std::true_type{});
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + c;
        if (q >= N) continue;
        T* row = dqkv + ((long)b * N + q) * 3 * H * HD + (long)(0 * H + h) * HD;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4<T>(row + dt * 16 + g * 4, dq[dt][qt] * scale);
    }
}

// ------------------------------------------------------------------------------------------ backward: dQ on an LDS-DMA ring (round 6)
// attn_bwd_dq_kernel with the K / V tiles on the forward's three-slot LDS-DMA ring (two tiles ahead, one counted vmcnt wait + one barrier per tile, no
// staging registers) and every LDS read inline asm, pipelined by hand under the MFMAs — the dK/dV kernel's recipe (attn_bwd_dkv_dma_kernel, below).
// Key rows past N are clamped to row N - 1 in the partial last tile (the register-staged kernel stages zeros): their dS is set to zero there, as before.
template <typename T>      // bf16 | f16
__global__ __launch_bounds__(256, 2) void attn_bwd_dq_dma_kernel(const T* qkv, const T* o, const T* dout, const float* lse, float* delta, T* dqkv, int N, int H,
                                                                 float scale) {
    typedef typename Mma<T>::Frag Frag;
    constexpr int TILE = 64 * 128;
    __shared__ __attribute__((aligned(16))) char smem[6 * TILE];      // K slots 0..2 | V slots 0..2
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int xb_, h, b;
    attn_block_coords(xb_, h, b);
    const int q0 = xb_ * 128 + wave * 32;
    const int npad = (N + 63) / 64 * 64;
    const long ld_b = (long)3 * H * HD * 2;
    const char* base = (const char*)qkv + (long)b * N * ld_b;
    const char* qb = base + (long)(0 * H + h) * HD * 2;
    const char* kb = base + (long)(1 * H + h) * HD * 2;
    const char* vb = base + (long)(2 * H + h) * HD * 2;
    const long ldo_b = (long)H * HD * 2;
    const char* dob = (const char*)dout + (long)b * N * ldo_b + (long)h * HD * 2;
    const char* ob = (const char*)o + (long)b * N * ldo_b + (long)h * HD * 2;

    // delta = rowsum(dO * O), from the dO fragments this wave loads anyway; left for the dK/dV kernel with -lse2 (see attn_bwd_dq_kernel)
    Frag qf[2][2], dof[2][2];
    f32x4 nlq[2], ndl[2];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + c;
        const bool ok = q < N;
        float dsum = 0.f;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            Frag z = {};
            qf[qt][u] = ok ? frag_scale<T>(load_nfrag<T>(qb + (long)q * ld_b, u, g), scale * 1.4426950408889634f) : z;   // exp2 domain
            dof[qt][u] = ok ? load_nfrag<T>(dob + (long)q * ldo_b, u, g) : z;
            const Frag of_ = ok ? load_nfrag<T>(ob + (long)q * ldo_b, u, g) : z;
            dsum += frag_dot(dof[qt][u], of_);
        }
        dsum += __shfl_xor(dsum, 16, 64);
        dsum += __shfl_xor(dsum, 32, 64);
        const float lq = ok ? lse[((long)b * H + h) * N + q] * 1.4426950408889634f : 0.f;   // log2 units
        if (g == 0 && q < npad) {
            const long wi = ((long)b * H + h) * npad + q;
            delta[wi] = ok ? -dsum : 0.f;
            delta[(long)gridDim.z * H * npad + wi] = ok ? -lq : -1e30f;
        }
        nlq[qt] = f32x4{-lq, -lq, -lq, -lq};
        ndl[qt] = f32x4{-dsum, -dsum, -dsum, -dsum};
    }
    f32x4 dq[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) dq[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // DMA: wave w moves pieces 2w, 2w + 1 (8 rows each) of the K tile and of the V tile: four operations per wave and tile
    const int prow = lane >> 3, pchunk = lane & 7;
    const char* kp[2];
    const char* vp_[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wave * 2 + i) * 8 + prow;
        const long off = (long)row * ld_b + ((pchunk ^ AT<T>::sw(row)) * 16);
        kp[i] = kb + off;
        vp_[i] = vb + off;
    }
    auto issue = [&](int k0, int slot) {
        if (k0 + 64 <= N) {
            const unsigned long t0 = (unsigned)k0 * (unsigned)ld_b;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kp[i] + t0),
                                                 (__attribute__((address_space(3))) void*)(smem + slot * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vp_[i] + t0),
                                                 (__attribute__((address_space(3))) void*)(smem + (3 + slot) * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
            }
            return;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (wave * 2 + i) * 8 + prow;
            const long off = (long)min(k0 + row, N - 1) * ld_b + ((pchunk ^ AT<T>::sw(row)) * 16);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(kb + off),
                                             (__attribute__((address_space(3))) void*)(smem + slot * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(vb + off),
                                             (__attribute__((address_space(3))) void*)(smem + (3 + slot) * TILE + (wave * 2 + i) * 1024), 16, 0, 0);
        }
    };
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)smem;
    const int swn = AT<T>::sw(c);
    const unsigned na0 = c * 128 + ((0 + g) ^ swn) * 16, na1 = c * 128 + ((4 + g) ^ swn) * 16;      // natural fragment (kt, u): row 16 kt + c, chunk 4u + g
    const int tq_ = c >> 2, tp = c & 3, swt = AT<T>::sw(4 * g + tq_);
    unsigned ta[4];                                                                                  // transposed fragment (dt, u): rows 32u + 4g + q (+16), chunk 2dt + (p >> 1)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ta[dt] = (4 * g + tq_) * 128 + (((2 * dt + (tp >> 1)) ^ swt) * 16) + 8 * (tp & 1);

    const int ntile = (N + 63) / 64;
    const bool live = q0 < N;      // a wave whose 32 queries are all past N only moves its DMA pieces
    issue(0, 0);
    if (ntile > 1) issue(64, 1);
    int slot = 0;
    auto key_tile = [&](int t, auto tail_tag) __attribute__((always_inline)) {
        constexpr bool tail = decltype(tail_tag)::value;
        if (t + 1 < ntile) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // tile t landed; tile t + 1 may still fly
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (t + 2 < ntile) issue((t + 2) * 64, slot == 0 ? 2 : slot - 1);
        const unsigned kbase = lds0 + slot * TILE, vbase = lds0 + (3 + slot) * TILE;
        slot = slot == 2 ? 0 : slot + 1;
        if (!live) return;
        // RK(kt): the K and V natural fragments of key tile kt; CK(kt): S / dP MFMAs + exp for it (both query tiles); RT(u, dt): the transposed K fragments
        // of head-dim tile dt for the 32 keys of half u; MQ(u, dt): its two dQ MFMAs.  Order (at most 12 reads outstanding):
        //   RK0 RK1 | CK0 | RK2 | CK1 | RT00 RT01 | MQ00 | RT02 | MQ01 | RT03 | MQ02 | RK3 | MQ03 | CK2 | CK3 | RT10 RT11 | MQ10 | RT12 | MQ11 | RT13 | MQ12 | MQ13
        const unsigned ka0 = kbase + na0, ka1 = kbase + na1, va0 = vbase + na0, va1 = vbase + na1;
        f32x4 rk0[2], rk1[2], rv0[2], rv1[2];
        a_u32x2 tr_[2][2];
        f32x4 ds[2][2];      // [query tile][key tile & 1]
        Frag df[2];
#define DQ_RK(kt, S) ADS_R128(rk0[S], ka0, kt * 2048); ADS_R128(rk1[S], ka1, kt * 2048); ADS_R128(rv0[S], va0, kt * 2048); ADS_R128(rv1[S], va1, kt * 2048);
#define DQ_WAIT_K(n, S) asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(rk0[S]), "+v"(rk1[S]), "+v"(rv0[S]), "+v"(rv1[S]) : "i"(n));
#define DQ_CK(kt, S)                                                                                                                    \
        _Pragma("unroll") for (int qt = 0; qt < 2; ++qt) {                                                                              \
            f32x4 sacc = nlq[qt], dpa = ndl[qt];                                                                                        \
            sacc = Mma<T>::mma(__builtin_bit_cast(Frag, rk0[S]), qf[qt][0], sacc);                                                      \
            dpa = Mma<T>::mma(__builtin_bit_cast(Frag, rv0[S]), dof[qt][0], dpa);                                                       \
            sacc = Mma<T>::mma(__builtin_bit_cast(Frag, rk1[S]), qf[qt][1], sacc);                                                      \
            dpa = Mma<T>::mma(__builtin_bit_cast(Frag, rv1[S]), dof[qt][1], dpa);                                                       \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                             \
                ds[qt][kt & 1][r] = fast_exp2(sacc[r]) * dpa[r];       /* the 1/sqrt(d) factor is applied once, to dQ */                \
                if (tail && t * 64 + kt * 16 + g * 4 + r >= N) ds[qt][kt & 1][r] = 0.f;                                                 \
            }                                                                                                                           \
        }
#define DQ_FRAGS()                                                                                                                      \
        _Pragma("unroll") for (int qt = 0; qt < 2; ++qt) { const f32x4 t4[4] = {ds[qt][0], ds[qt][1], ds[qt][0], ds[qt][1]}; df[qt] = acc_to_bfrag<T>(t4, 0); }
#define DQ_RT(u, dt, S) ADS_TR64(tr_[S][0], kbase + ta[dt], u * 4096); ADS_TR64(tr_[S][1], kbase + ta[dt], u * 4096 + 2048);
#define DQ_WAIT_T(n, S) asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(tr_[S][0]), "+v"(tr_[S][1]) : "i"(n));
#define DQ_MQ(dt, S)                                                                                                                    \
        {                                                                                                                               \
            typedef __attribute__((ext_vector_type(4))) unsigned a_u32x4;                                                               \
            const a_u32x4 z = {tr_[S][0][0], tr_[S][0][1], tr_[S][1][0], tr_[S][1][1]};                                                 \
            const Frag kt_ = __builtin_bit_cast(Frag, z);                                                                               \
            _Pragma("unroll") for (int qt = 0; qt < 2; ++qt) dq[dt][qt] = Mma<T>::mma(kt_, df[qt], dq[dt][qt]);                         \
        }
        DQ_RK(0, 0) DQ_RK(1, 1)
        DQ_WAIT_K(4, 0) DQ_CK(0, 0)
        DQ_RK(2, 0)
        DQ_WAIT_K(4, 1) DQ_CK(1, 1)
        DQ_FRAGS()
        DQ_RT(0, 0, 0) DQ_RT(0, 1, 1)
        DQ_WAIT_T(2, 0) DQ_MQ(0, 0)
        DQ_RT(0, 2, 0)
        DQ_WAIT_T(2, 1) DQ_MQ(1, 1)
        DQ_RT(0, 3, 1)
        DQ_WAIT_T(2, 0) DQ_MQ(2, 0)
        DQ_RK(3, 1)
        DQ_WAIT_T(4, 1) DQ_MQ(3, 1)
        DQ_WAIT_K(4, 0) DQ_CK(2, 0)
        DQ_WAIT_K(0, 1) DQ_CK(3, 1)
        DQ_FRAGS()
        DQ_RT(1, 0, 0) DQ_RT(1, 1, 1)
        DQ_WAIT_T(2, 0) DQ_MQ(0, 0)
        DQ_RT(1, 2, 0)
        DQ_WAIT_T(2, 1) DQ_MQ(1, 1)
        DQ_RT(1, 3, 1)
        DQ_WAIT_T(2, 0) DQ_MQ(2, 0)
        DQ_WAIT_T(0, 1) DQ_MQ(3, 1)
#undef DQ_RK
#undef DQ_WAIT_K
#undef DQ_CK
#undef DQ_FRAGS
#undef DQ_RT
#undef DQ_WAIT_T
#undef DQ_MQ
    };
    {
        int t = 0;
        for (; (t + 1) * 64 <= N; ++t) key_tile(t, std::false_type{});
        if (t * 64 < N) key_tile(t, std::true_type{});
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        const int q = q0 + qt * 16 + c;
        if (q >= N) continue;
        T* row = dqkv + ((long)b * N + q) * 3 * H * HD + (long)(0 * H + h) * HD;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) store4<T>(row + dt * 16 + g * 4, dq[dt][qt] * scale);
    }
}

// ------------------------------------------------------------------------------------------ backward: dK, dV
// DK = false: dV only (the first trainable block of the student: nothing below it learns, so dK — and with it dP, dS and the Q^T
// operand — is never used; half of the kernel's MFMAs)
template <typename T, int NW, bool DK = true>
__global__ __launch_bounds__(64 * NW, (NW >= 8 || IsX3<T>::v) ? 1 : 2) void attn_bwd_dkv_kernel(const T* qkv, const T* dout, const float* lse,
                                                           const float* delta, T* dqkv, int N, int H, float scale, int vfirst) {
    vfirst &= 0xff;
    constexpr int NF = AT<T>::NF, ROWB = AT<T>::ROWB;
    typedef typename Mma<T>::Frag Frag;
    __shared__ __attribute__((aligned(16))) char sQ[64 * ROWB];
    __shared__ __attribute__((aligned(16))) char sQt[TSZ(T)];
    __shared__ __attribute__((aligned(16))) char sD[64 * ROWB];
    __shared__ __attribute__((aligned(16))) char sDt[TSZ(T)];
    __shared__ __attribute__((aligned(16))) float sL[64], sDl[64];   // -lse (log2 units) and -delta of the tile's 64 queries
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, c = lane & 15;
    constexpr int NT = 64 * NW;
    int xb_, h, b;
    attn_block_coords(xb_, h, b);
    const int key0 = xb_ * (32 * NW) + wave * 32;
    const long ld_b = (long)3 * H * HD * sizeof(T);
    const char* base = (const char*)qkv + (long)b * N * ld_b;
    const char* qb = base + (long)(0 * H + h) * HD * sizeof(T);
    const char* kb = base + (long)(1 * H + h) * HD * sizeof(T);
    const char* vb = base + (long)(2 * H + h) * HD * sizeof(T);
    const long ldo_b = (long)H * HD * sizeof(T);
    const char* dob = (const char*)dout + (long)b * N * ldo_b + (long)h * HD * sizeof(T);

    Frag kf[2][NF], vf[2][NF];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + kt * 16 + c;
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            Frag z = {};
            kf[kt][u] = key < N ? frag_scale<T>(load_nfrag<T>(kb + (long)key * ld_b, u, g), scale * 1.4426950408889634f) : z;   // exp2 domain
            vf[kt][u] = key < N ? load_nfrag<T>(vb + (long)key * ld_b, u, g) : z;
        }
    }
    const bool wave_live = key0 < N;
    f32x4 dk[4][2], dv[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) { dk[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    const int ntile = (N + 63) / 64;
    auto pq0 = [&](int t) { return t * 64; };
    TileRegs<T, NT> rq, rd;
    TileSrc<T, NT> qsrc, dsrc;
    tile_src_init<T, NT>(qsrc, qb, ld_b, N);
    tile_src_init<T, NT>(dsrc, dob, ldo_b, N);
    tile_load<T, NT>(rq, qsrc, pq0(0));
    tile_load<T, NT>(rd, dsrc, pq0(0));
    float rl = 0.f, rdl = 0.f;   // next tile's -lse (log2 units) / -delta rows, prefetched with the tile
    // the dQ kernel left them in that form in `delta` = ws [2][B * H][npad] (ws[0] = -delta, ws[1] = -lse2), padded to whole tiles: queries >= N have
    // -lse2 = -1e30, i.e. p = 2^(s - 1e30) = 0 (their Q / dO rows are staged as zeros) — no mask in the loop.  (`lse` itself is not read here any more.)
    const int npad = (N + 63) / 64 * 64;
    const float* wsd = delta + ((long)b * H + h) * npad;
    const float* wsl = delta + (long)gridDim.z * H * npad + ((long)b * H + h) * npad;
    if (threadIdx.x < 64) {
        const int q = pq0(0) + threadIdx.x;
        rl = wsl[q];
        rdl = wsd[q];
    }
    for (int t = 0; t < ntile; ++t) {
        __syncthreads();
        tile_store<T, true, TOp<T>::kNeedT, NT>(rq, sQ, sQt);
        tile_store<T, true, TOp<T>::kNeedT, NT>(rd, sD, sDt);
        if (t + 1 < ntile) {
            tile_load<T, NT>(rq, qsrc, pq0(t + 1));
            tile_load<T, NT>(rd, dsrc, pq0(t + 1));
        }
        if (threadIdx.x < 64) { sL[threadIdx.x] = rl; sDl[threadIdx.x] = rdl; }   // (already negated: accumulator seeds)
        if (t + 1 < ntile && threadIdx.x < 64) {
            const int q = pq0(t + 1) + threadIdx.x;
            rl = wsl[q];
            rdl = wsd[q];
        }
        __syncthreads();
        if (!wave_live) continue;   // (this wave's 32 keys are all past N: it only helps staging the tiles — 5 of the 48 waves of an
                                    //  (image, head) at N = 1370)
        f32x4 pp[2][4], dsv[2][4];  // [key tile][query tile]
#pragma unroll
        for (int qt = 0; qt < 4; ++qt) {
            Frag qf[NF], df[NF];
#pragma unroll
            for (int u = 0; u < NF; ++u) {
                qf[u] = lds_nfrag<T>(sQ, qt * 16 + c, u, g);
                if (DK) df[u] = lds_nfrag<T>(sD, qt * 16 + c, u, g);
            }
            // row constants as the initial accumulators: the four queries 16 qt + 4 g + r of this lane's C rows
            const f32x4 nl = *(const f32x4*)(sL + qt * 16 + g * 4), nd = *(const f32x4*)(sDl + qt * 16 + g * 4);
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) {
                f32x4 s = nl, dp = nd;
#pragma unroll
                for (int u = 0; u < NF; ++u) {
                    s = Mma<T>::mma(qf[u], kf[kt][u], s);    // rows: queries, cols: keys
                    if (DK) dp = Mma<T>::mma(df[u], vf[kt][u], dp);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = fast_exp2(s[r]);
                    pp[kt][qt][r] = p;
                    if (DK) dsv[kt][qt][r] = p * dp[r];            // the 1/sqrt(d) factor is applied once, to dK
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NF; ++u) {
            Frag pf[2], sf[2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt) { pf[kt] = acc_to_bfrag<T>(pp[kt], u); if (DK) sf[kt] = acc_to_bfrag<T>(dsv[kt], u); }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const Frag dot = TOp<T>::load(sD, sDt, dt, u, g, lane);
                Frag qt_ = dot;
                if (DK) qt_ = TOp<T>::load(sQ, sQt, dt, u, g, lane);
#pragma unroll
                for (int kt = 0; kt < 2; ++kt) {
                    dv[dt][kt] = Mma<T>::mma(dot, pf[kt], dv[dt][kt]);
                    if (DK) dk[dt][kt] = Mma<T>::mma(qt_, sf[kt], dk[dt][kt]);
                }
            }
        }
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + kt * 16 + c;
        if (key >= N) continue;
        // column block of dK / dV inside the packed gradient row: (dq, dk, dv) or, with vfirst, (dq, dv, dk)
        T* rk = dqkv + ((long)b * N + key) * 3 * H * HD + (long)((vfirst ? 2 : 1) * H + h) * HD;
        T* rv = dqkv + ((long)b * N + key) * 3 * H * HD + (long)((vfirst ? 1 : 2) * H + h) * HD;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            if (DK) store4<T>(rk + dt * 16 + g * 4, dk[dt][kt] * scale);
            store4<T>(rv + dt * 16 + g * 4, dv[dt][kt]);
        }
    }
}

// ------------------------------------------------------------------------------------------ backward: dK, dV on an LDS-DMA ring (round 6)
// attn_bwd_dkv_kernel<T, 4> spends 27 % of its time staging the Q / dO tiles (anatomy, profiles/r06_probe_attn_tn.txt: buffer loads into registers ->
// ds_write -> two block barriers per 64-query tile; 255 of 935 us at 64 x 12 x 1370).  Here the tiles — and the tile's 64 + 64 row constants, which
// the dQ kernel leaves negated and in log2 units in ws — travel global -> LDS by LDS-DMA into a THREE-slot ring, two tiles ahead, as in
// attn_fwd_dma_kernel: no staging registers, no ds_write, no address arithmetic on the vector ALU for full tiles, ONE counted vmcnt wait and ONE barrier
// per tile.  Same mathematics, register layouts and swizzle (chunk ^ AT<T>::sw(row), applied on the SOURCE address) as the register-staged kernel; every
// LDS read of the ring is inline asm (a ds_read the compiler can see gets an `s_waitcnt vmcnt(0)` to the LDS-DMA in flight in front of it).
// Query rows past N are clamped to row N - 1 in the partial last tile: their -lse2 is -1e30 (ws pads), so p = 0 and dS = 0 * finite = 0.
template <typename T, bool DK = true>      // bf16 | f16; four waves = 128 keys per block
__global__ __launch_bounds__(256, 2) void attn_bwd_dkv_dma_kernel(const T* qkv, const T* dout, const float* ws, T* dqkv, int N, int H, float scale, int vfirst) {
    typedef typename Mma<T>::Frag Frag;
    constexpr int TILE = 64 * 128;                    // one Q or dO tile: 64 rows x 128 B
    constexpr int SLOT = 2 * TILE + 512;              // Q tile | dO tile | -lse2 [64] | -delta [64]
    __shared__ __attribute__((aligned(16))) char smem[3 * SLOT];
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int xb_, h, b;
    attn_block_coords(xb_, h, b);
    const int key0 = xb_ * 128 + wave * 32;
    const long ld_b = (long)3 * H * HD * 2;
    const char* base = (const char*)qkv + (long)b * N * ld_b;
    const char* qb = base + (long)(0 * H + h) * HD * 2;
    const char* kb = base + (long)(1 * H + h) * HD * 2;
    const char* vb = base + (long)(2 * H + h) * HD * 2;
    const long ldo_b = (long)H * HD * 2;
    const char* dob = (const char*)dout + (long)b * N * ldo_b + (long)h * HD * 2;
    const int npad = (N + 63) / 64 * 64;
    const float* wsd = ws + ((long)b * H + h) * npad;                                         // -delta
    const float* wsl = ws + (long)gridDim.z * H * npad + ((long)b * H + h) * npad;            // -lse (log2 units)

    Frag kf[2][2], vf[2][2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + kt * 16 + c;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            Frag z = {};
            kf[kt][u] = key < N ? frag_scale<T>(load_nfrag<T>(kb + (long)key * ld_b, u, g), scale * 1.4426950408889634f) : z;   // exp2 domain
            vf[kt][u] = key < N ? load_nfrag<T>(vb + (long)key * ld_b, u, g) : z;
        }
    }
    const bool wave_live = key0 < N;
    f32x4 dk[4][2], dv[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) { dk[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    // DMA: wave w moves pieces 2w, 2w + 1 (8 rows each) of the Q tile and of the dO tile, and one 256-byte piece of row constants (even waves -lse2,
    // odd waves -delta; waves 2 / 3 repeat what 0 / 1 send — the same bytes to the same place — so that every wave counts FIVE operations per tile)
    const int prow = lane >> 3, pchunk = lane & 7;
    const char* qp[2];
    const char* dp_[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wave * 2 + i) * 8 + prow;
        qp[i] = qb + (long)row * ld_b + ((pchunk ^ AT<T>::sw(row)) * 16);
        dp_[i] = dob + (long)row * ldo_b + ((pchunk ^ AT<T>::sw(row)) * 16);
    }
    const float* cp = ((wave & 1) ? wsd : wsl) + lane;
    const int coff = 2 * TILE + (wave & 1) * 256;
    auto issue = [&](int q0t, int slot) {
        char* sb = smem + slot * SLOT;
        if (q0t + 64 <= N) {
            const unsigned long tq = (unsigned)q0t * (unsigned)ld_b, td = (unsigned)q0t * (unsigned)ldo_b;     // (an image's rows span < 2^31 bytes)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(qp[i] + tq),
                                                 (__attribute__((address_space(3))) void*)(sb + (wave * 2 + i) * 1024), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(dp_[i] + td),
                                                 (__attribute__((address_space(3))) void*)(sb + TILE + (wave * 2 + i) * 1024), 16, 0, 0);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = (wave * 2 + i) * 8 + prow;
                const long r = min(q0t + row, N - 1);
                const int sw16 = (pchunk ^ AT<T>::sw(row)) * 16;
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(qb + r * ld_b + sw16),
                                                 (__attribute__((address_space(3))) void*)(sb + (wave * 2 + i) * 1024), 16, 0, 0);
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(dob + r * ldo_b + sw16),
                                                 (__attribute__((address_space(3))) void*)(sb + TILE + (wave * 2 + i) * 1024), 16, 0, 0);
            }
        }
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(cp + q0t),
                                         (__attribute__((address_space(3))) void*)(sb + coff), 4, 0, 0);
    };
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) const void*)smem;
    // natural fragment (qt, u): row qt * 16 + c, logical chunk 4u + g (row qt * 16 + c has the swizzle of row c)
    const int swn = AT<T>::sw(c);
    const unsigned na0 = c * 128 + ((0 + g) ^ swn) * 16, na1 = c * 128 + ((4 + g) ^ swn) * 16;
    // transposed fragment (dt, u): rows 32u + 4g + q (+16), logical chunk 2dt + (p >> 1), 8-byte half p & 1
    const int tq_ = c >> 2, tp = c & 3, swt = AT<T>::sw(4 * g + tq_);
    unsigned ta[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) ta[dt] = (4 * g + tq_) * 128 + (((2 * dt + (tp >> 1)) ^ swt) * 16) + 8 * (tp & 1);
    const unsigned ca = 2 * TILE + g * 16;            // the four row constants 16 qt + 4g + r of this lane's C rows: one b128 at +64 qt

    const int ntile = (N + 63) / 64;
    issue(0, 0);
    if (ntile > 1) issue(64, 1);
    int slot = 0;
    for (int t = 0; t < ntile; ++t) {
        if (t + 1 < ntile) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");   // tile t landed; tile t + 1 may still fly
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();            // everyone's pieces of tile t landed; everyone is done with tile t - 1's slot
        asm volatile("" ::: "memory");
        if (t + 2 < ntile) issue((t + 2) * 64, slot == 0 ? 2 : slot - 1);
        const unsigned sbase = lds0 + slot * SLOT;
        slot = slot == 2 ? 0 : slot + 1;
        if (!wave_live) continue;   // (this wave's 32 keys are all past N: it only moves its DMA pieces)
        // ---- the tile, software-pipelined by hand over the LDS reads (inline asm reads are invisible to the scheduler; at most 14 are outstanding:
        // lgkmcnt counts to 15).  RA(qt): the natural fragments + row constants of query tile qt; CA(qt): S / dP MFMAs + exp for it; RT(u, dt): the
        // transposed dO / Q fragments of head-dim tile dt for the 32 queries of half u; MB(u, dt): its four dV / dK MFMAs.  Order:
        //   RA0 RA1 | CA0 | RA2 | CA1 | RT00 RT01 | MB00 | RT02 | MB01 | RT03 | MB02 | RA3 | MB03 | CA2 | CA3 | RT10 RT11 | MB10 | RT12 | MB11 | RT13 | MB12 | MB13
        const unsigned qa0 = sbase + na0, qa1 = sbase + na1, da0 = sbase + TILE + na0, da1 = sbase + TILE + na1, cb = sbase + ca;
        const unsigned dtb = sbase + TILE, qtb = sbase;
        f32x4 aq0[2], aq1[2], ad0[2], ad1[2], anl[2], and_[2];      // two register sets for RA
        a_u32x2 tdr[2][2], tqr[2][2];                               // two register sets for RT: [set][row half]
        f32x4 pp[2][2], dsv[2][2];                                   // [key tile][query tile & 1]: two query tiles at a time
        Frag pf[2], sf[2];
        constexpr int NRA = DK ? 6 : 3, NRT = DK ? 4 : 2;            // LDS reads per RA / RT
#define DKV_RA(qt, S)                                                                                                                   \
        ADS_R128(aq0[S], qa0, qt * 2048); ADS_R128(aq1[S], qa1, qt * 2048); ADS_R128(anl[S], cb, qt * 64);                           \
        if (DK) { ADS_R128(ad0[S], da0, qt * 2048); ADS_R128(ad1[S], da1, qt * 2048); ADS_R128(and_[S], cb, 256 + qt * 64); }
#define DKV_WAIT_A(n, S)                                                                                                                \
        if (DK) asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(aq0[S]), "+v"(aq1[S]), "+v"(ad0[S]), "+v"(ad1[S]), "+v"(anl[S]), "+v"(and_[S]) : "i"(n)); \
        else asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(aq0[S]), "+v"(aq1[S]), "+v"(anl[S]) : "i"(n));
#define DKV_CA(qt, S)                                                                                                                   \
        {                                                                                                                               \
            const Frag qf0 = __builtin_bit_cast(Frag, aq0[S]), qf1 = __builtin_bit_cast(Frag, aq1[S]);                                  \
            _Pragma("unroll") for (int kt = 0; kt < 2; ++kt) {                                                                          \
                f32x4 sacc = anl[S], dpa = anl[S];                                                                                      \
                sacc = Mma<T>::mma(qf0, kf[kt][0], sacc);    /* rows: queries, cols: keys */                                            \
                sacc = Mma<T>::mma(qf1, kf[kt][1], sacc);                                                                               \
                if (DK) {                                                                                                               \
                    dpa = and_[S];                                                                                                      \
                    dpa = Mma<T>::mma(__builtin_bit_cast(Frag, ad0[S]), vf[kt][0], dpa);                                                \
                    dpa = Mma<T>::mma(__builtin_bit_cast(Frag, ad1[S]), vf[kt][1], dpa);                                                \
                }                                                                                                                       \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                                         \
                    const float pv = fast_exp2(sacc[r]);                                                                                \
                    pp[kt][qt & 1][r] = pv;                                                                                             \
                    if (DK) dsv[kt][qt & 1][r] = pv * dpa[r];          /* the 1/sqrt(d) factor is applied once, to dK */                \
                }                                                                                                                       \
            }                                                                                                                           \
        }
        // the B fragments of half u from the two query tiles just computed (contraction index = 16 (qt & 1) + 4g + r within the half)
#define DKV_FRAGS()                                                                                                                     \
        _Pragma("unroll") for (int kt = 0; kt < 2; ++kt) {                                                                              \
            const f32x4 t4[4] = {pp[kt][0], pp[kt][1], pp[kt][0], pp[kt][1]};                                                           \
            pf[kt] = acc_to_bfrag<T>(t4, 0);                                                                                            \
            if (DK) { const f32x4 d4[4] = {dsv[kt][0], dsv[kt][1], dsv[kt][0], dsv[kt][1]}; sf[kt] = acc_to_bfrag<T>(d4, 0); }          \
        }
#define DKV_RT(u, dt, S)                                                                                                                \
        ADS_TR64(tdr[S][0], dtb + ta[dt], u * 4096); ADS_TR64(tdr[S][1], dtb + ta[dt], u * 4096 + 2048);                              \
        if (DK) { ADS_TR64(tqr[S][0], qtb + ta[dt], u * 4096); ADS_TR64(tqr[S][1], qtb + ta[dt], u * 4096 + 2048); }
#define DKV_WAIT_T(n, S)                                                                                                                \
        if (DK) asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(tdr[S][0]), "+v"(tdr[S][1]), "+v"(tqr[S][0]), "+v"(tqr[S][1]) : "i"(n));    \
        else asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(tdr[S][0]), "+v"(tdr[S][1]) : "i"(n));
#define DKV_MB(dt, S)                                                                                                                   \
        {                                                                                                                               \
            typedef __attribute__((ext_vector_type(4))) unsigned a_u32x4;                                                               \
            const a_u32x4 zd = {tdr[S][0][0], tdr[S][0][1], tdr[S][1][0], tdr[S][1][1]};                                                \
            const Frag dot = __builtin_bit_cast(Frag, zd);                                                                              \
            _Pragma("unroll") for (int kt = 0; kt < 2; ++kt) dv[dt][kt] = Mma<T>::mma(dot, pf[kt], dv[dt][kt]);                         \
            if (DK) {                                                                                                                   \
                const a_u32x4 zq = {tqr[S][0][0], tqr[S][0][1], tqr[S][1][0], tqr[S][1][1]};                                            \
                const Frag qt_ = __builtin_bit_cast(Frag, zq);                                                                          \
                _Pragma("unroll") for (int kt = 0; kt < 2; ++kt) dk[dt][kt] = Mma<T>::mma(qt_, sf[kt], dk[dt][kt]);                     \
            }                                                                                                                           \
        }
        DKV_RA(0, 0) DKV_RA(1, 1)
        DKV_WAIT_A(NRA, 0) DKV_CA(0, 0)
        DKV_RA(2, 0)
        DKV_WAIT_A(NRA, 1) DKV_CA(1, 1)
        DKV_FRAGS()
        DKV_RT(0, 0, 0) DKV_RT(0, 1, 1)
        DKV_WAIT_T(NRT, 0) DKV_MB(0, 0)            // (RA2 is older than the RTs: it has landed too)
        DKV_RT(0, 2, 0)
        DKV_WAIT_T(NRT, 1) DKV_MB(1, 1)
        DKV_RT(0, 3, 1)
        DKV_WAIT_T(NRT, 0) DKV_MB(2, 0)
        DKV_RA(3, 1)
        DKV_WAIT_T(NRA, 1) DKV_MB(3, 1)
        DKV_WAIT_A(NRA, 0) DKV_CA(2, 0)            // (landed long ago: the wait only ties the registers)
        DKV_WAIT_A(0, 1) DKV_CA(3, 1)
        DKV_FRAGS()
        DKV_RT(1, 0, 0) DKV_RT(1, 1, 1)
        DKV_WAIT_T(NRT, 0) DKV_MB(0, 0)
        DKV_RT(1, 2, 0)
        DKV_WAIT_T(NRT, 1) DKV_MB(1, 1)
        DKV_RT(1, 3, 1)
        DKV_WAIT_T(NRT, 0) DKV_MB(2, 0)
        DKV_WAIT_T(0, 1) DKV_MB(3, 1)
#undef DKV_RA
#undef DKV_WAIT_A
#undef DKV_CA
#undef DKV_FRAGS
#undef DKV_RT
#undef DKV_WAIT_T
#undef DKV_MB
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
        const int key = key0 + kt * 16 + c;
        if (key >= N) continue;
        // column block of dK / dV inside the packed gradient row: (dq, dk, dv) or, with vfirst, (dq, dv, dk)
        T* rk = dqkv + ((long)b * N + key) * 3 * H * HD + (long)((vfirst ? 2 : 1) * H + h) * HD;
        T* rv = dqkv + ((long)b * N + key) * 3 * H * HD + (long)((vfirst ? 1 : 2) * H + h) * HD;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            if (DK) store4<T>(rk + dt * 16 + g * 4, dk[dt][kt] * scale);
            store4<T>(rv + dt * 16 + g * 4, dv[dt][kt]);
        }
    }
}

// ------------------------------------------------------------------------------------------ C ABI
template <typename T> constexpr bool kIs16 = std::is_same<T, bf16>::value || std::is_same<T, f16>::value;

// the element type of a dtype code, handed to `f` as a null pointer of that type (GD_F16 = the tf32h engine: fp16 q / k / v / p with TF32's significand on
// the bf16 kernels' layouts; in the backward dout arrives times a power of two, the caller's gd_amax_scale, and dqkv leaves with it)
template <typename F> static void attn_with_type(int dtype, F f) {
    if (dtype == GD_BF16) f((bf16*)nullptr);
    else if (dtype == GD_F16) f((f16*)nullptr);
    else if (dtype == GD_F32X3) f((x3*)nullptr);
    else f((float*)nullptr);
}

template <typename T>
static void attn_fwd_launch(const void* qkv, void* o, float* lse, int B, int N, int H, float scale, hipStream_t s) {
    const dim3 grid(gd_cdiv(N, 128), H, B);
    if constexpr (kIs16<T>) {
        if (gd_knobs().attn_dma) {      // GD_ATTN_DMA=0: the register-staged forward kernel (A/B testing)
            hipLaunchKernelGGL(attn_fwd_dma_kernel<T>, grid, dim3(256), 0, s, (const T*)qkv, (T*)o, lse, N, H, scale, gd_knobs().attn_rot);
            return;
        }
    }
    hipLaunchKernelGGL(attn_fwd_kernel<T>, grid, dim3(256), 0, s, (const T*)qkv, (T*)o, lse, N, H, scale);
}

extern "C" int gd_attention_fwd(const void* qkv, void* o, float* lse, int B, int N, int H, int head_dim, float scale,
                                int dtype, void* stream) {
    GD_REQUIRE(B > 0 && N > 0 && H > 0, "gd_attention_fwd: bad shape B=%d N=%d H=%d", B, N, H);
    GD_REQUIRE(head_dim == HD, "gd_attention_fwd: head_dim must be 64 (got %d)", head_dim);
    GD_REQUIRE((long)N * 3 * H * HD * 4 < (1L << 31), "gd_attention_fwd: one image's qkv rows must span < 2^31 bytes (32-bit tile offsets): N=%d H=%d", N, H);
    GD_REQUIRE(dtype == GD_F32 || dtype == GD_BF16 || dtype == GD_F32X3 || dtype == GD_F16, "gd_attention_fwd: bad dtype %d", dtype);
    GD_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)o & 15) == 0, "gd_attention_fwd: pointers must be 16-byte aligned");
    attn_with_type(dtype, [&](auto* t) { attn_fwd_launch<std::remove_pointer_t<decltype(t)>>(qkv, o, lse, B, N, H, scale, (hipStream_t)stream); });
    GD_LAUNCH_OK();
    return 0;
}

// Which dK/dV kernel runs: 32 keys per wave, `waves` waves per block (4 | 8); `dma`: the four-wave LDS-DMA kernel (16-bit operands only).
struct DkvForm { int waves; bool dma; };
// opt_nw = GD_ATTN_DKV_NW (0 auto | 4 | 8: forces one form), opt_dma = GD_ATTN_DKV_DMA (0: the register-staged kernels, A/B).
static DkvForm attn_dkv_form(int dtype, int N, int opt_nw, int opt_dma) {
    if (dtype == GD_F32) return {8, false};
    if (dtype == GD_F32X3) return {4, false};      // the whole register file per wave (the (hi, lo) fragments double the operand registers)
    // 16-bit: 128-key blocks of four waves (two blocks per CU, independent barriers, Q / dO tiles staged twice as often) when the last
    // 256-key block would be less than half full: N = 1370 pads to 1408 keys instead of 1536 (2.7 % instead of 10.8 %):
    // backward 1574 -> 1514 us at 64 x 12 x 1370; at N = 6401 (long sweeps, 0.4 % vs 2 % padding) the 8-wave form is 2 % faster.
    // (two-wave 64-key blocks: 2213 us — the staging registers spill and every block re-stages all of Q / dO)
    const int tail = N % 256;
    const int waves = opt_nw ? opt_nw : ((N < 4096 && tail > 0 && tail <= 128) ? 4 : 8);
    return {waves, waves == 4 && opt_dma != 0};
}

struct AttnBwdArgs {
    const void *qkv, *o, *dout;
    const float* lse;
    void* dqkv;
    float* ws;
    int B, N, H;
    float scale;
    int vfirst;
    hipStream_t s;
};
template <typename T, int NW, bool DK> static void attn_dkv_launch_regs(const AttnBwdArgs& a) {
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<T, NW, DK>), dim3(gd_cdiv(a.N, 32 * NW), a.H, a.B), dim3(64 * NW), 0, a.s, (const T*)a.qkv, (const T*)a.dout, a.lse,
                       a.ws, (T*)a.dqkv, a.N, a.H, a.scale, a.vfirst);
}
// (only the forms attn_dkv_form can return for T are instantiated)
template <typename T, bool DK> static void attn_dkv_launch(const AttnBwdArgs& a, DkvForm f) {
    if constexpr (kIs16<T>) {
        if (f.dma) {
            hipLaunchKernelGGL((attn_bwd_dkv_dma_kernel<T, DK>), dim3(gd_cdiv(a.N, 128), a.H, a.B), dim3(256), 0, a.s, (const T*)a.qkv, (const T*)a.dout, a.ws,
                               (T*)a.dqkv, a.N, a.H, a.scale, a.vfirst);
            return;
        }
    }
    if constexpr (std::is_same<T, float>::value) attn_dkv_launch_regs<T, 8, DK>(a);
    else if constexpr (IsX3<T>::v) attn_dkv_launch_regs<T, 4, DK>(a);
    else if (f.waves == 4) attn_dkv_launch_regs<T, 4, DK>(a);
    else attn_dkv_launch_regs<T, 8, DK>(a);
}
template <typename T> static void attn_bwd_launch(const AttnBwdArgs& a, DkvForm f, bool no_dk) {
    const dim3 grid(gd_cdiv(a.N, 128), a.H, a.B);
    bool dq_dma = false;
    if constexpr (kIs16<T>) {
        dq_dma = gd_knobs().attn_dq_dma != 0;      // GD_ATTN_DQ_DMA=0: the register-staged kernel (A/B)
        if (dq_dma) hipLaunchKernelGGL(attn_bwd_dq_dma_kernel<T>, grid, dim3(256), 0, a.s, (const T*)a.qkv, (const T*)a.o, (const T*)a.dout, a.lse, a.ws, (T*)a.dqkv, a.N, a.H, a.scale);
    }
    if (!dq_dma) hipLaunchKernelGGL(attn_bwd_dq_kernel<T>, grid, dim3(256), 0, a.s, (const T*)a.qkv, (const T*)a.o, (const T*)a.dout, a.lse, a.ws, (T*)a.dqkv, a.N, a.H, a.scale);
    // the exact-f32 kernel has no dV-only form: it computes dK whether or not it is needed
    if constexpr (std::is_same<T, float>::value) attn_dkv_launch<T, true>(a, f);
    else if (no_dk) attn_dkv_launch<T, false>(a, f);
    else attn_dkv_launch<T, true>(a, f);
}

// delta_ws of gd_attention_bwd: [2][B * H][Npad] floats (-delta | -lse2), Npad = N rounded up to whole 64-query tiles (what the kernels call npad)
extern "C" size_t gd_attention_bwd_workspace_bytes(int B, int N, int H) {
    if (B <= 0 || N <= 0 || H <= 0) return 0;
    const size_t npad = ((size_t)N + 63) / 64 * 64;
    return 2 * (size_t)B * (size_t)H * npad * sizeof(float);
}

extern "C" int gd_attention_bwd(const void* qkv, const void* o, const void* dout, const float* lse, void* dqkv,
                                float* delta_ws, int B, int N, int H, int head_dim, float scale, int dtype,
                                int grad_order, void* stream) {
    GD_REQUIRE(grad_order >= 0 && grad_order <= 3, "gd_attention_bwd: grad_order bit 0: 0 = (dq, dk, dv), 1 = (dq, dv, dk); bit 1: dK not needed");
    GD_REQUIRE(B > 0 && N > 0 && H > 0, "gd_attention_bwd: bad shape B=%d N=%d H=%d", B, N, H);
    GD_REQUIRE(head_dim == HD, "gd_attention_bwd: head_dim must be 64 (got %d)", head_dim);
    GD_REQUIRE((long)N * 3 * H * HD * 4 < (1L << 31), "gd_attention_bwd: one image's qkv rows must span < 2^31 bytes (32-bit tile offsets): N=%d H=%d", N, H);
    GD_REQUIRE(dtype == GD_F32 || dtype == GD_BF16 || dtype == GD_F32X3 || dtype == GD_F16, "gd_attention_bwd: bad dtype %d", dtype);
    GD_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)dout & 15) == 0 && ((uintptr_t)dqkv & 15) == 0,
               "gd_attention_bwd: pointers must be 16-byte aligned");
    GD_REQUIRE(((uintptr_t)o & 15) == 0, "gd_attention_bwd: o must be 16-byte aligned");
    const AttnBwdArgs a = {qkv, o, dout, lse, dqkv, delta_ws, B, N, H, scale, grad_order & 1, (hipStream_t)stream};
    const DkvForm f = attn_dkv_form(dtype, N, gd_knobs().attn_dkv_nw, gd_knobs().attn_dkv_dma);
    const bool no_dk = (grad_order & 2) != 0;
    attn_with_type(dtype, [&](auto* t) { attn_bwd_launch<std::remove_pointer_t<decltype(t)>>(a, f, no_dk); });
    GD_LAUNCH_OK();
    return 0;
}
