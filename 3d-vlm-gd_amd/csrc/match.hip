// Correspondence evaluation (src/evaluate_timm.py): the similarity argmax of the OnePose++ matcher in both directions
// (:166-179) and the argmax over the upsampled, edge-padded score field of the semantic transfer (:531-547).  Neither
// the M x N similarity matrix nor the upsampled feature map reaches memory.
#include "gemm_tile.h"
#include "argmax_keys.h"     // packed (score, ~index) keys and their lane / wave reductions

// ---------------------------------------------------------------------------------------------------------------------
// Fused similarity argmax: one 128 x 128 tile of S = A . B^T per block on the shared MFMA main loop (gemm_tile.h), and an
// epilogue that reduces the tile's accumulators to a key per row (over the tile's 128 columns) and per column (over its 128
// rows): within the lane, across the 16 (row) / 4 (column) lanes that share it, across the two waves through LDS, then one
// vector 64-bit atomic max per row and per column into rkeys / ckeys.
// acc[i][j][r] of wave (wm, wn) is S[tm*128 + wm*64 + 16 i + 4 (lane >> 4) + r][tn*128 + wn*64 + 16 j + (lane & 15)].
// ---------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void match_argmax_kernel(const T* A, const T* B, int M, int N, int D, int mt,
                                                           unsigned long long* rkeys, unsigned long long* ckeys) {
    __shared__ __attribute__((aligned(16))) char smem[GD_TILE_SMEM];
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = bid % mt, tn = bid / mt;       // consecutive blocks share a B panel and walk A (the smaller operand)
    f32x4 acc[4][4];
    const long ldb = (long)D * sizeof(T);
    mma_tile_128x128<T>((const char*)A, ldb, M, (const char*)B, ldb, N, (int)ldb, tm, tn, smem, acc);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
    const int rl0 = wm * 64 + 4 * (lane >> 4), cl0 = wn * 64 + (lane & 15);     // tile-local row / column of acc[0][0][0]
    const int r0 = tm * 128 + rl0, c0 = tn * 128 + cl0;
    unsigned long long* srow = (unsigned long long*)smem;    // [wn][128]: the main loop ended on a barrier, smem is free
    unsigned long long* scol = srow + 256;                   // [wm][128]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned long long best = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = acc[i][j][r];
                if (c0 + 16 * j < N) best = umax64(best, gd_key(v, c0 + 16 * j));
            }
            best = row16_max_u64(best);
            if ((lane & 15) == 0) srow[wn * 128 + rl0 + 16 * i + r] = best;
        }
    if (ckeys) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            unsigned long long best = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = acc[i][j][r];
                    if (r0 + 16 * i + r < M) best = umax64(best, gd_key(v, r0 + 16 * i + r));
                }
            best = umax64(best, __shfl_xor(best, 16, 64));
            best = umax64(best, __shfl_xor(best, 32, 64));
            if (lane < 16) scol[wm * 128 + cl0 + 16 * j] = best;
        }
    }
    __syncthreads();
    const int t = threadIdx.x & 127;
    if (threadIdx.x < 128) {
        const int row = tm * 128 + t;
        if (row < M) atomicMax(rkeys + row, umax64(srow[t], srow[128 + t]));
    } else if (ckeys) {
        const int col = tn * 128 + t;
        if (col < N) atomicMax(ckeys + col, umax64(scol[t], scol[128 + t]));
    }
}

// keys -> int64 indices (and scores times the operands' inverse scales); mutual[i] = (col_idx[row_idx[i]] == i)
__global__ void match_decode_kernel(const unsigned long long* rkeys, const unsigned long long* ckeys, int M, int N,
                                    const float* inv_a, const float* inv_b, long long* row_idx, float* row_score,
                                    long long* col_idx, float* col_score, unsigned char* mutual) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    const float sc = (inv_a ? *inv_a : 1.f) * (inv_b ? *inv_b : 1.f);
    if (t < M) {
        const unsigned long long k = rkeys[t];
        const int j = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
        row_idx[t] = j;
        if (row_score) row_score[t] = gd_unord((unsigned)(k >> 32)) * sc;
        if (mutual) mutual[t] = (j >= 0 && j < N && (int)(0xFFFFFFFFu - (unsigned)(ckeys[j] & 0xFFFFFFFFull)) == t) ? 1 : 0;
    }
    if (ckeys && t < N) {
        const unsigned long long k = ckeys[t];
        col_idx[t] = (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull));
        if (col_score) col_score[t] = gd_unord((unsigned)(k >> 32)) * sc;
    }
}

static size_t gd_align256(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" size_t gd_match_argmax_workspace_bytes(int M, int N, int flags) {
    if (M <= 0 || N <= 0) return 0;
    return gd_align256((size_t)M * 8) + ((flags & GD_MATCH_COLS) ? gd_align256((size_t)N * 8) : 0);
}

extern "C" int gd_match_argmax(const void* A, const void* B, int M, int N, int D, int dtype, int flags, const float* inv_scale_a,
                               const float* inv_scale_b, long long* row_idx, float* row_score, long long* col_idx, float* col_score,
                               unsigned char* mutual, void* workspace, void* stream) {
    GD_REQUIRE(M > 0 && N > 0 && D > 0 && D % 8 == 0, "gd_match_argmax: need M, N > 0 and D a positive multiple of 8 (M=%d N=%d D=%d)", M, N, D);
    GD_REQUIRE(dtype == GD_F32 || dtype == GD_F16 || dtype == GD_BF16, "gd_match_argmax: bad dtype %d", dtype);
    GD_REQUIRE((flags & ~GD_MATCH_COLS) == 0, "gd_match_argmax: unknown flags 0x%x", flags);
    const bool cols = (flags & GD_MATCH_COLS) != 0;
    GD_REQUIRE(A && B && row_idx && workspace, "gd_match_argmax: A, B, row_idx and workspace are required");
    GD_REQUIRE(cols || (!col_idx && !col_score && !mutual), "gd_match_argmax: col_idx / col_score / mutual need flags GD_MATCH_COLS");
    GD_REQUIRE(!cols || col_idx, "gd_match_argmax: GD_MATCH_COLS needs col_idx");
    GD_REQUIRE(((uintptr_t)A & 15) == 0 && ((uintptr_t)B & 15) == 0, "gd_match_argmax: A and B must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* rkeys = (unsigned long long*)workspace;
    unsigned long long* ckeys = cols ? (unsigned long long*)((char*)workspace + gd_align256((size_t)M * 8)) : nullptr;
    GD_REQUIRE(hipMemsetAsync(workspace, 0, gd_match_argmax_workspace_bytes(M, N, flags), s) == hipSuccess, "gd_match_argmax: memset failed");
    const int mt = gd_cdiv(M, 128), nt = gd_cdiv(N, 128);
    GD_REQUIRE((long)mt * nt < (1L << 31), "gd_match_argmax: %d x %d tiles exceed the grid", mt, nt);
    const dim3 grid((unsigned)(mt * nt));
    if (dtype == GD_F32)
        hipLaunchKernelGGL(match_argmax_kernel<float>, grid, dim3(256), 0, s, (const float*)A, (const float*)B, M, N, D, mt, rkeys, ckeys);
    else if (dtype == GD_F16)
        hipLaunchKernelGGL(match_argmax_kernel<f16>, grid, dim3(256), 0, s, (const f16*)A, (const f16*)B, M, N, D, mt, rkeys, ckeys);
    else
        hipLaunchKernelGGL(match_argmax_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)A, (const bf16*)B, M, N, D, mt, rkeys, ckeys);
    hipLaunchKernelGGL(match_decode_kernel, dim3(gd_cdiv(cols ? (M > N ? M : N) : M, 256)), dim3(256), 0, s, rkeys, ckeys, M, N,
                       inv_scale_a, inv_scale_b, row_idx, row_score, col_idx, col_score, mutual);
    GD_LAUNCH_OK();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Semantic-transfer argmax: the field is S[k] upsampled to (ds_h, ds_w), ds = ((img - patch) // stride) * stride + 1, by
// torch's bilinear align_corners=True arithmetic (upsample_bilinear2d: fp32 scale (in - 1) / (out - 1), source = scale * dst,
// integer part + lambda, the nested lerp), then edge-padded by patch // 2 on the top / left.  Every one of the img_h x img_w
// pixels is evaluated (plateaus in the padding and near-ties between nodes resolve as the materialised field does); per
// block one key per k (raster index, first occurrence on ties), combined across blocks by a vector 64-bit atomic max.
// S[k][y * pitch + x], x < gw: the K x (gh x gw) score grid (pitch >= gw columns per grid line in memory).
// ---------------------------------------------------------------------------------------------------------------------
#define TA_PIX 4096
__global__ __launch_bounds__(256) void transfer_argmax_kernel(const float* S, int gh, int gw, int pitch, int img_h, int img_w,
                                                              int ds_h, int ds_w, int pad, unsigned long long* keys) {
    __shared__ unsigned long long part[4];
    const int k = blockIdx.y;
    const float* s = S + (long)k * gh * pitch;
    const float rh = ds_h > 1 ? (float)(gh - 1) / (float)(ds_h - 1) : 0.f;
    const float rw = ds_w > 1 ? (float)(gw - 1) / (float)(ds_w - 1) : 0.f;
    const long npix = (long)img_h * img_w, p0 = (long)blockIdx.x * TA_PIX;
    unsigned long long best = 0;
    for (int q = threadIdx.x; q < TA_PIX; q += 256) {
        const long pix = p0 + q;
        if (pix >= npix) break;
        const int y = (int)(pix / img_w), x = (int)(pix % img_w);
        const int yy = min(max(y - pad, 0), ds_h - 1), xx = min(max(x - pad, 0), ds_w - 1);
        const float h1r = rh * (float)yy, w1r = rw * (float)xx;
        const int h1 = (int)h1r, w1 = (int)w1r;
        const int h1p = h1 < gh - 1 ? pitch : 0, w1p = w1 < gw - 1 ? 1 : 0;
        const float h1l = h1r - (float)h1, h0l = 1.f - h1l, w1l = w1r - (float)w1, w0l = 1.f - w1l;
        const float* c = s + (long)h1 * pitch + w1;
        const float v = h0l * (w0l * c[0] + w1l * c[w1p]) + h1l * (w0l * c[h1p] + w1l * c[h1p + w1p]);
        best = umax64(best, gd_key(v, (int)pix));
    }
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(keys + k, umax64(umax64(part[0], part[1]), umax64(part[2], part[3])));
}
__global__ void transfer_decode_kernel(const unsigned long long* keys, int K, int img_w, long long* xy, float* score) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const long long idx = (long long)(0xFFFFFFFFu - (unsigned)(keys[k] & 0xFFFFFFFFull));
    xy[2 * k] = idx % img_w;
    xy[2 * k + 1] = idx / img_w;
    if (score) score[k] = gd_unord((unsigned)(keys[k] >> 32));
}

extern "C" size_t gd_transfer_argmax_workspace_bytes(int K) { return K > 0 ? gd_align256((size_t)K * 8) : 0; }

extern "C" int gd_transfer_argmax(const float* S, int K, int gh, int gw, int pitch, int img_h, int img_w, int patch, int stride,
                                  long long* xy, float* score, void* workspace, void* stream) {
    GD_REQUIRE(S && xy && workspace, "gd_transfer_argmax: S, xy and workspace are required");
    GD_REQUIRE(K > 0 && gh > 0 && gw > 0 && pitch >= gw && patch > 0 && stride > 0 && img_h >= patch && img_w >= patch,
               "gd_transfer_argmax: bad arguments (K=%d grid %dx%d pitch %d image %dx%d patch %d stride %d)", K, gh, gw, pitch, img_h, img_w, patch, stride);
    GD_REQUIRE(K <= 65535, "gd_transfer_argmax: at most 65535 queries per call (got %d)", K);
    GD_REQUIRE((long)img_h * img_w < (1L << 31), "gd_transfer_argmax: image %dx%d too large", img_h, img_w);
    GD_REQUIRE(gh == 1 + (img_h - patch) / stride && gw == 1 + (img_w - patch) / stride,
               "gd_transfer_argmax: grid %dx%d is not 1 + (image - patch) // stride for image %dx%d, patch %d, stride %d", gh, gw, img_h, img_w, patch, stride);
    const int ds_h = ((img_h - patch) / stride) * stride + 1, ds_w = ((img_w - patch) / stride) * stride + 1;
    hipStream_t s = (hipStream_t)stream;
    GD_REQUIRE(hipMemsetAsync(workspace, 0, (size_t)K * 8, s) == hipSuccess, "gd_transfer_argmax: memset failed");
    hipLaunchKernelGGL(transfer_argmax_kernel, dim3(gd_cdiv((long)img_h * img_w, TA_PIX), K), dim3(256), 0, s, S, gh, gw, pitch, img_h, img_w,
                       ds_h, ds_w, patch / 2, (unsigned long long*)workspace);
    hipLaunchKernelGGL(transfer_decode_kernel, dim3(gd_cdiv(K, 256)), dim3(256), 0, s, (const unsigned long long*)workspace, K, img_w, xy, score);
    GD_LAUNCH_OK();
    return 0;
}
