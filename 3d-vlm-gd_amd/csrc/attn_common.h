// What more than one attention translation unit needs (attention.hip, cross_view_attn.hip): the MFMA operand traits of the four element types,
// the fragment helpers, the 64-row LDS tile layouts with their register-staged loads / stores, the softmax helpers and the inline-asm LDS reads of
// the LDS-DMA kernels.  Every object that includes this header is built with -fno-slp-vectorize (Makefile).
#pragma once
#include "gd_common.h"
#include <type_traits>
#include <stdlib.h>

#define HD 64

// ---- split-precision path (dtype code GD_F32X3): fp32 tensors in memory, every MFMA operand as a (hi, lo) pair of bf16 fragments,
// hi = bf16(x), lo = bf16(x - hi), and every product as the three bf16 MFMAs  lo_a hi_b + hi_a lo_b + hi_a hi_b  (all of a . b except
// lo_a lo_b: ~4e-6 relative, TF32 ~3e-4) — 3 x 16 MFMA cycles per 32-wide chunk against 8 x 32 for the exact-f32 MFMA.  The same
// kernels, instantiated on the tag type `x3` (a 4-byte element: pointer arithmetic is fp32's); only the traits below differ.
struct x3 { float v; };
struct X3Frag { bf16x8 hi, lo; };
template <typename T> struct IsX3 { static constexpr bool v = false; };
template <> struct IsX3<x3> { static constexpr bool v = true; };
template <> struct Mma<x3> {
    static constexpr int KC = 32;
    typedef X3Frag Frag;
    static __device__ __forceinline__ f32x4 mma(const Frag& a, const Frag& b, f32x4 c) {
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.lo, b.hi, c, 0, 0, 0);      // small terms first
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.lo, c, 0, 0, 0);
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.hi, b.hi, c, 0, 0, 0);
    }
};
__device__ __forceinline__ X3Frag x3_split(const float (&x)[8]) {
    X3Frag f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        f.hi[k] = (bf16)x[k];
        f.lo[k] = (bf16)(x[k] - (float)f.hi[k]);
    }
    return f;
}
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }   // bare v_exp_f32
// max over the 4 lanes {l, l^16, l^32, l^48} with the gfx950 row-swap instructions (VALU; a ds_bpermute pair costs two
// dependent LDS round trips in the middle of the softmax)
// (The two results of a swap are taken out as SCALARS before they are reinterpreted: __builtin_bit_cast applied to an ext-vector element
// expression a[1] reads element 0 on ROCm 7.2's clang — rounds 1-3 shipped `fmaxf(bit_cast(a[0]), bit_cast(a[1]))`, which compiled to a[0] alone:
// every lane got lane group 0's maximum instead of the query's.  A uniform but arbitrary reference point still gives the right o and lse — which
// is why every bf16 / f32 test passed — but it does not bound p by 2^ATT_THR, and fp16 p overflowed to inf on peaked rows: found by round 4's
// adversarial fp16 cases, tests/test_gpu_attention.py::test_attention_reference_point_moves[float16].)
__device__ __forceinline__ float quad_rows_max(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const unsigned a0 = a[0], a1 = a[1];
    v = fmaxf(__builtin_bit_cast(float, a0), __builtin_bit_cast(float, a1));
    const unsigned w = __builtin_bit_cast(unsigned, v);
    const auto b = __builtin_amdgcn_permlane32_swap(w, w, false, false);
    const unsigned b0 = b[0], b1 = b[1];
    return fmaxf(__builtin_bit_cast(float, b0), __builtin_bit_cast(float, b1));
}

// ---- softmax with a LAGGED reference point (forward) ---------------------------------------------------------------
// The score accumulators are started from -m (the MFMA's C operand: a persistent register quartet per query tile, no
// instruction), with q pre-multiplied by scale*log2(e), so a finished accumulator is already  s*c2 - m  and p is ONE
// v_exp per score — the online softmax's subtract / scale FMA is gone, and so is its running row sum: the row sums come
// out of the PV product as one more MFMA per k-chunk against an all-ones A fragment (they are then the sums of exactly
// the bf16-rounded p that multiply V).  m is a reference point, not the exact running maximum: the first tile sets it to
// the tile's row maximum, later tiles only RAISE it, and only when a score exceeds it by more than ATT_THR (p <= 2^THR
// otherwise): a wave-uniform branch that is almost never taken after the first tiles.  Any reference point gives the same
// o = sum p v / sum p and lse = m + log2 sum p; the first-tile rule keeps sum p >= 1, so nothing can underflow to 0 / 0.
#ifndef ATT_THR
#define ATT_THR 8.0f
#endif
// the two 16-bit element types share every layout: bf16 (bf16 engine) and fp16 (tf32h engine: TF32's significand; conversions saturate)
template <typename T> struct V16;
template <> struct V16<bf16> { typedef bf16x8 T8; typedef bf16x4 T4; };
template <> struct V16<f16> { typedef f16x8 T8; typedef f16x4 T4; };
template <typename T> __device__ __forceinline__ typename Mma<T>::Frag frag_scale(typename Mma<T>::Frag f, float a);
template <typename T> __device__ __forceinline__ typename V16<T>::T8 frag_scale16(typename V16<T>::T8 f, float a) {
    typename V16<T>::T8 o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = from_f32<T>((float)f[k] * a);
    return o;
}
template <> __device__ __forceinline__ bf16x8 frag_scale<bf16>(bf16x8 f, float a) { return frag_scale16<bf16>(f, a); }
template <> __device__ __forceinline__ f16x8 frag_scale<f16>(f16x8 f, float a) { return frag_scale16<f16>(f, a); }
template <> __device__ __forceinline__ f32x4 frag_scale<float>(f32x4 f, float a) { return f * a; }
template <> __device__ __forceinline__ X3Frag frag_scale<x3>(X3Frag f, float a) {      // scale the fp32 value, split again
    float x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = ((float)f.hi[k] + (float)f.lo[k]) * a;
    return x3_split(x);
}
template <typename T> __device__ __forceinline__ typename Mma<T>::Frag frag_ones();
template <> __device__ __forceinline__ bf16x8 frag_ones<bf16>() {
    const bf16 o = (bf16)1.0f;
    return bf16x8{o, o, o, o, o, o, o, o};
}
template <> __device__ __forceinline__ f16x8 frag_ones<f16>() {
    const f16 o = (f16)1.0f;
    return f16x8{o, o, o, o, o, o, o, o};
}
template <> __device__ __forceinline__ f32x4 frag_ones<float>() { return f32x4{1.f, 1.f, 1.f, 1.f}; }
template <> __device__ __forceinline__ X3Frag frag_ones<x3>() {
    X3Frag f = {};
    f.hi = frag_ones<bf16>();
    return f;
}

// s[qt][kt] hold s*c2 - m of a 64-key tile (TAIL: keys >= N get -1e30).  Updates m / negm (and rescales o, l) when the
// tile's maximum moved the reference point, then turns the scores into p in place.
template <bool TAIL>
__device__ __forceinline__ void softmax_lagged(f32x4 (&s)[2][4], float (&m)[2], f32x4 (&negm)[2], f32x4 (&oacc)[4][2],
                                               f32x4 (&lacc)[2], bool first, int k0, int g, int N) {
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
        float tmax = -1e30f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (TAIL && k0 + kt * 16 + g * 4 + r >= N) s[qt][kt][r] = -1e30f;
                tmax = fmaxf(tmax, s[qt][kt][r]);
            }
        // the cross-lane maximum is only needed when SOME lane of the wave sees a score above the threshold (if no lane's own 16 scores exceed
        // it, no query's 64 do): the steady state pays one compare and a wave-uniform branch, not the two lane exchanges
        if (first || __any(tmax > ATT_THR)) {
            tmax = quad_rows_max(tmax);
            const bool need = first || tmax > ATT_THR;
            const float d = need ? tmax : 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) s[qt][kt][r] -= d;
            m[qt] += d;
            negm[qt] = f32x4{-m[qt], -m[qt], -m[qt], -m[qt]};
            if (!first) {                                  // (first tile: o and l are still zero, and d may be negative)
                const float alpha = fast_exp2(-d);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) oacc[dt][qt] *= alpha;
                lacc[qt] *= alpha;
            }
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[qt][kt][r] = fast_exp2(s[qt][kt][r]);
    }
}

template <typename T> struct AT;
// LDS tiles of 64 rows.  bf16: rows are 128 bytes UNPADDED and the 16-byte chunk index is XOR-ed with
// sw(row) = ((row >> 1) & 3) << 1.  One image serves both read patterns conflict-free (PMC before: 33-43 % of the LDS cycles
// of these kernels were bank-conflict cycles with padded 144-byte rows / the GEMM's (row >> 1) & 7 swizzle):
//   * ds_read_b128 fragment reads (rows 16 k + c, chunk 4 u + g): the hardware serves lanes {0-3, 12-15, 20-27} together —
//     rows c in {0..3, 12..15} at chunk q and rows {4..11} at chunk q ^ 1; rows of equal parity share a 128-byte bank
//     half and get the XOR values {0, 2, 4, 6} resp. {4, 6, 0, 2}: eight distinct chunks per half;
//   * ds_read_b64_tr_b16 transpose reads (32 lanes = 8 consecutive rows x the chunk PAIR {2 dt, 2 dt + 1}): the four rows of
//     equal parity need four different pairs — XOR by an even number that differs between them, which an odd XOR ((row >> 1) & 7
//     has them) does not give.
struct AT16 {
    static constexpr int NF = 2;        // fragments per 64-wide contraction
    static constexpr int ROWB = 128;    // LDS row: 64 el * 2 B
    static constexpr int CPR = 8;       // 16-byte chunks per 64-element row
    static constexpr int EPC = 8;       // elements per chunk
    static __device__ __forceinline__ int sw(int row) { return ((row >> 1) & 3) << 1; }
};
template <> struct AT<bf16> : AT16 {};
template <> struct AT<f16> : AT16 {};
template <> struct AT<float> {
    static constexpr int NF = 4;
    static constexpr int ROWB = 272;    // 64 el * 4 B + 16 pad, linear
    static constexpr int CPR = 16;
    static constexpr int EPC = 4;
    static __device__ __forceinline__ int sw(int) { return 0; }
};

// x3: an LDS row is 256 bytes = 16 positions of 16 bytes: plane pl (0 hi, 1 lo), chunk q (8 bf16 each) sits at position
// (8 pl + q) ^ (row & 15) — the sixteen rows 16 k + c that a ds_read_b128 lane group reads at one logical chunk land on sixteen
// different positions; row and row + 16 share the swizzle (the transpose reads rely on it).
template <> struct AT<x3> {
    static constexpr int NF = 2;        // (hi, lo) fragment pairs per 64-wide contraction
    static constexpr int ROWB = 256;
    static constexpr int CPR = 16;      // 16-byte chunks per 64-float GLOBAL row
    static constexpr int EPC = 4;
    static __device__ __forceinline__ int sw(int row) { return row & 15; }
};

// four C-layout tiles that span 64 contraction indices (index = 16*tile + 4*g + r) -> B fragment u
template <typename T> __device__ __forceinline__ typename Mma<T>::Frag acc_to_bfrag(const f32x4 (&t)[4], int u);
template <> __device__ __forceinline__ bf16x8 acc_to_bfrag<bf16>(const f32x4 (&t)[4], int u) {
    const f32x4 a = t[2 * u], b = t[2 * u + 1];
    return bf16x8{(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
}
template <> __device__ __forceinline__ f16x8 acc_to_bfrag<f16>(const f32x4 (&t)[4], int u) {
    const f32x4 a = t[2 * u], b = t[2 * u + 1];
    // plain conversions (v_cvt_pk_f16_f32; a saturating clamp per element made these issue-port-bound kernels 13-26 % slower): p <= 2^ATT_THR
    // in the forward, p <= 1 and |dS| <= |dP - delta| in the backward, where dP is a 64-term dot product of the SCALED dout (|dout| s <= 8,
    // vit.py) with v — five orders of magnitude below 65504 for any realistic v
    return f16x8{(f16)a[0], (f16)a[1], (f16)a[2], (f16)a[3], (f16)b[0], (f16)b[1], (f16)b[2], (f16)b[3]};
}
template <> __device__ __forceinline__ f32x4 acc_to_bfrag<float>(const f32x4 (&t)[4], int u) { return t[u]; }
template <> __device__ __forceinline__ X3Frag acc_to_bfrag<x3>(const f32x4 (&t)[4], int u) {
    const f32x4 a = t[2 * u], b = t[2 * u + 1];
    const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return x3_split(x);
}

// matching A fragment from a transposed LDS tile row (64 contraction indices contiguous)
template <typename T> __device__ __forceinline__ typename Mma<T>::Frag load_tfrag(const char* row, int u, int g);
template <> __device__ __forceinline__ bf16x8 load_tfrag<bf16>(const char* row, int u, int g) {
    const bf16x4 a = *(const bf16x4*)(row + (32 * u + 4 * g) * 2);
    const bf16x4 b = *(const bf16x4*)(row + (32 * u + 16 + 4 * g) * 2);
    return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
template <> __device__ __forceinline__ f16x8 load_tfrag<f16>(const char* row, int u, int g) {
    const f16x4 a = *(const f16x4*)(row + (32 * u + 4 * g) * 2);
    const f16x4 b = *(const f16x4*)(row + (32 * u + 16 + 4 * g) * 2);
    return f16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}
template <> __device__ __forceinline__ f32x4 load_tfrag<float>(const char* row, int u, int g) {
    return *(const f32x4*)(row + (16 * u + 4 * g) * 4);
}

// natural fragment u (16 bytes) of a [row][64] LDS tile row / global row
template <typename T> __device__ __forceinline__ typename Mma<T>::Frag load_nfrag(const char* row, int u, int g) {
    return *(const typename Mma<T>::Frag*)(row + u * 64 + g * 16);
}

// natural fragment u of row `row` of an LDS tile (chunk 4 u + g, swizzled)
template <typename T> __device__ __forceinline__ typename Mma<T>::Frag lds_nfrag(const char* tile, int row, int u, int g) {
    return *(const typename Mma<T>::Frag*)(tile + row * AT<T>::ROWB + (((u * 4 + g) ^ AT<T>::sw(row)) * 16));
}

template <> __device__ __forceinline__ X3Frag load_nfrag<x3>(const char* row, int u, int g) {      // GLOBAL fp32 row: floats 32 u + 8 g .. + 7
    const f32x4 a = *(const f32x4*)(row + (32 * u + 8 * g) * 4), b = *(const f32x4*)(row + (32 * u + 8 * g + 4) * 4);
    const float x[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return x3_split(x);
}
template <> __device__ __forceinline__ X3Frag lds_nfrag<x3>(const char* tile, int row, int u, int g) {
    const char* r = tile + row * AT<x3>::ROWB;
    X3Frag f;
    f.hi = *(const bf16x8*)(r + (((u * 4 + g) ^ AT<x3>::sw(row)) * 16));
    f.lo = *(const bf16x8*)(r + (((8 + u * 4 + g) ^ AT<x3>::sw(row)) * 16));
    return f;
}

// Tile staging, split T14-style: `tile_load` issues the global loads of a 64 x 64-element tile into registers
// (rows >= nvalid read as zero) and `tile_store` writes them to LDS later — as a natural tile sN[row][64]
// and/or a transposed tile sT[col][row] — so the next tile's HBM/L2 latency hides under the current tile's MFMAs.
template <typename T, int NT = 256> struct TileRegs { uint4 v[AT<T>::CPR * 64 / NT]; };

template <typename T, int NT = 256>
__device__ __forceinline__ void tile_load(TileRegs<T, NT>& r, const char* gbase, long ld_b, int row0, int nvalid) {
    constexpr int CPR = AT<T>::CPR, NCH = CPR * 64 / NT;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = threadIdx.x + NT * i, rr = ch / CPR, cc = ch % CPR;
        r.v[i] = (row0 + rr < nvalid) ? *(const uint4*)(gbase + (long)(row0 + rr) * ld_b + cc * 16) : make_uint4(0, 0, 0, 0);
    }
}
// The same through a buffer resource (backward kernels): rows >= nvalid lie past the resource's last record and read as zero
// in hardware — no per-chunk compare / exec mask / zero-fill and no 64-bit address arithmetic in the tile loop (that was 28 of the
// dQ loop's 76 non-transcendental VALU instructions); the per-thread byte offsets are loop-invariant, the tile adds row0 * ld.
template <typename T, int NT = 256> struct TileSrc {
    __amdgpu_buffer_rsrc_t rs;
    int off[AT<T>::CPR * 64 / NT];
    int ld;
};
template <typename T, int NT = 256>
__device__ __forceinline__ void tile_src_init(TileSrc<T, NT>& src, const char* gbase, long ld_b, int nvalid) {
    constexpr int CPR = AT<T>::CPR, NCH = CPR * 64 / NT;
    src.rs = __builtin_amdgcn_make_buffer_rsrc((void*)gbase, (short)0, (int)((long)(nvalid - 1) * ld_b + 64 * (long)sizeof(T)), 0x00020000);
    src.ld = (int)ld_b;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = threadIdx.x + NT * i, rr = ch / CPR, cc = ch % CPR;
        src.off[i] = rr * (int)ld_b + cc * 16;
    }
}
template <typename T, int NT = 256>
__device__ __forceinline__ void tile_load(TileRegs<T, NT>& r, const TileSrc<T, NT>& src, int row0) {
    constexpr int NCH = AT<T>::CPR * 64 / NT;
    const int base = row0 * src.ld;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
        r.v[i] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(src.rs, src.off[i] + base, 0, 0));
}
template <typename T, bool NAT, bool TRN, int NT = 256>
__device__ __forceinline__ void tile_store(const TileRegs<T, NT>& r, char* sN, char* sT) {
    constexpr int CPR = AT<T>::CPR, EPC = AT<T>::EPC, ROWB = AT<T>::ROWB, NCH = CPR * 64 / NT;
    if constexpr (std::is_same<T, x3>::value) {      // four floats -> four hi + four lo bf16 (8 bytes each): half `cc & 1` of bf16 chunk `cc >> 1`
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int ch = threadIdx.x + NT * i, rr = ch / CPR, cc = ch % CPR;
            const f32x4 x = __builtin_bit_cast(f32x4, r.v[i]);
            bf16x4 hi, lo;
#pragma unroll
            for (int k = 0; k < 4; ++k) { hi[k] = (bf16)x[k]; lo[k] = (bf16)(x[k] - (float)hi[k]); }
            char* row = sN + rr * ROWB + 8 * (cc & 1);
            *(bf16x4*)(row + (((cc >> 1) ^ AT<x3>::sw(rr)) * 16)) = hi;
            *(bf16x4*)(row + (((8 + (cc >> 1)) ^ AT<x3>::sw(rr)) * 16)) = lo;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
        const int ch = threadIdx.x + NT * i, rr = ch / CPR, cc = ch % CPR;
        if (NAT) *(uint4*)(sN + rr * ROWB + ((cc ^ AT<T>::sw(rr)) * 16)) = r.v[i];
        if (TRN) {
            const T* e = (const T*)&r.v[i];
#pragma unroll
            for (int k = 0; k < EPC; ++k) *(T*)(sT + (cc * EPC + k) * ROWB + rr * (int)sizeof(T)) = e[k];
        }
    }
}

// The "transposed operand" A[row = column c of the tile][k-slot = tile row]:
//   bf16: read straight from the NATURAL tile with ds_read_b64_tr_b16 (hardware 4x16 transpose per 16-lane group:
//         lane 4q+p supplies the address of block row q, columns 4p..4p+3; lane i receives column i of the 4 rows)
//   f32 : 16-byte read from an explicitly transposed LDS tile.
template <typename T> struct TOp;
template <typename T> struct TOp16 {
    static constexpr bool kNeedT = false;
    static __device__ __forceinline__ typename V16<T>::T8 load(const char* sN, const char*, int dt, int u, int g, int lane) {
        typedef __attribute__((ext_vector_type(4))) short s16x4;
        const int i = lane & 15, q = i >> 2, p = i & 3;
        const int row = 32 * u + 4 * g + q;                         // (row + 16 has the same swizzle)
        const char* a0 = sN + row * AT<bf16>::ROWB + (((2 * dt + (p >> 1)) ^ AT<bf16>::sw(row)) * 16) + 8 * (p & 1);
        const char* a1 = a0 + 16 * AT<bf16>::ROWB;
        const s16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
        const s16x4 y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a1);
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        const s16x8 z = {x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
        return __builtin_bit_cast(typename V16<T>::T8, z);
    }
};
template <> struct TOp<bf16> : TOp16<bf16> {};
template <> struct TOp<f16> : TOp16<f16> {};
template <> struct TOp<x3> {      // both planes straight from the natural tile, as bf16
    static constexpr bool kNeedT = false;
    static __device__ __forceinline__ bf16x8 plane(const char* sN, int pl, int dt, int u, int g, int lane) {
        typedef __attribute__((ext_vector_type(4))) short s16x4;
        typedef __attribute__((ext_vector_type(8))) short s16x8;
        const int i = lane & 15, q = i >> 2, p = i & 3;
        const int row = 32 * u + 4 * g + q;                         // (row + 16 has the same swizzle)
        const char* a0 = sN + row * AT<x3>::ROWB + (((8 * pl + 2 * dt + (p >> 1)) ^ AT<x3>::sw(row)) * 16) + 8 * (p & 1);
        const char* a1 = a0 + 16 * AT<x3>::ROWB;
        const s16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a0);
        const s16x4 y = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)a1);
        const s16x8 z = {x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
        return __builtin_bit_cast(bf16x8, z);
    }
    static __device__ __forceinline__ X3Frag load(const char* sN, const char*, int dt, int u, int g, int lane) {
        X3Frag f;
        f.hi = plane(sN, 0, dt, u, g, lane);
        f.lo = plane(sN, 1, dt, u, g, lane);
        return f;
    }
};
template <> struct TOp<float> {
    static constexpr bool kNeedT = true;
    static __device__ __forceinline__ f32x4 load(const char*, const char* sT, int dt, int u, int g, int lane) {
        return load_tfrag<float>(sT + (dt * 16 + (lane & 15)) * AT<float>::ROWB, u, g);
    }
};
#define TSZ(T) (TOp<T>::kNeedT ? 64 * AT<T>::ROWB : 16)

template <typename T> __device__ __forceinline__ void store4(T* p, f32x4 v);
template <> __device__ __forceinline__ void store4<float>(float* p, f32x4 v) { *(f32x4*)p = v; }
template <> __device__ __forceinline__ void store4<x3>(x3* p, f32x4 v) { *(f32x4*)p = v; }
template <> __device__ __forceinline__ void store4<bf16>(bf16* p, f32x4 v) {
    *(bf16x4*)p = bf16x4{(bf16)v[0], (bf16)v[1], (bf16)v[2], (bf16)v[3]};
}
template <> __device__ __forceinline__ void store4<f16>(f16* p, f32x4 v) {
    *(f16x4*)p = f16_sat4(v[0], v[1], v[2], v[3]);
}


// dot of two operand fragments (the 16 bytes a lane holds of a row), fp32
__device__ __forceinline__ float frag_dot(bf16x8 a, bf16x8 b) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = fmaf((float)a[k], (float)b[k], s);
    return s;
}
__device__ __forceinline__ float frag_dot(f16x8 a, f16x8 b) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = fmaf((float)a[k], (float)b[k], s);
    return s;
}
__device__ __forceinline__ float frag_dot(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }
__device__ __forceinline__ float frag_dot(const X3Frag& a, const X3Frag& b) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s = fmaf((float)a.hi[k] + (float)a.lo[k], (float)b.hi[k] + (float)b.lo[k], s);
    return s;
}

// (x-block, head, image) of this workgroup.  The x-blocks of one (image, head) all sweep the same K / V (or Q / dO) rows;
// in plain launch order they are dealt round-robin over the eight XCDs, so every XCD's L2 pulls every (image, head)'s
// operands over the fabric (PMC: 2.2-2.5 GB per launch against 0.4-0.5 GB of operands).  The linear launch index is
// re-mapped so that each XCD gets a contiguous run of (image, head) groups, x-block fastest.
__device__ __forceinline__ void attn_block_coords(int& xb, int& h, int& b) {
    const int nx = gridDim.x, ny = gridDim.y;
    const int lin = blockIdx.x + nx * (blockIdx.y + ny * blockIdx.z);
    const int r = xcd_remap(lin, nx * ny * gridDim.z);
    xb = r % nx;
    h = (r / nx) % ny;
    b = r / (nx * ny);
}

// ---- inline-asm LDS reads of the LDS-DMA kernels (a ds_read the compiler can see gets an `s_waitcnt vmcnt` to the most recent LDS-DMA in front of
// it).  The offset is a compile-time expression: slot * tile size + row-group offset on one address register per lane.
#define ADS_R128(dst, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(imm))
#define ADS_TR64(dst, addr, imm) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(imm))
typedef __attribute__((ext_vector_type(2))) unsigned a_u32x2;
