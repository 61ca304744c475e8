// TAP-Vid tracking evaluation (src/evaluate_timm.py:234-348 on utils/tracking_model.py): the tracker head of one embedding
// against one frame — cosine map, relu, first argmax, soft-argmax over the disc of `radius` pixels around it (:147-200,
// :292-308) — for lists of up to 128 embeddings that share a target frame.  The per-row score map never reaches memory.
#include "gemm_tile.h"
#include "argmax_keys.h"

// ---------------------------------------------------------------------------------------------------------------------
// ||x_r|| in fp32 for every row of X [rows, D] (the reference's frame_embeddings_set.norm(dim=1) / source_embeddings.norm(dim=1)):
// one wave per row, lane-strided sum of squares, then a fixed butterfly, so the result repeats bit for bit.
// ---------------------------------------------------------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(256) void track_row_norms_kernel(const S* X, long rows, int D, float* out) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const S* x = X + row * D;
    float s = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float v = to_f32<S>(x[k]);
        s = fmaf(v, v, s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) out[row] = sqrtf(s);
}

// four consecutive elements of a row as fp32 (k a multiple of 4, D a multiple of 8: never straddles the row's end)
__device__ __forceinline__ f32x4 load4_f32(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 load4_f32(const f16* p) {
    const f16x4 h = *(const f16x4*)p;
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}
__device__ __forceinline__ f32x4 load4_f32(const bf16* p) {
    const bf16x4 h = *(const bf16x4*)p;
    return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

// ---------------------------------------------------------------------------------------------------------------------
// One block per tile {frame, row0, nrows, out0}: rows E[row0 .. row0 + nrows) against the gh x pitch cells of frame `frame`.
// Phase 1 walks every 128-column tile of the frame on the shared MFMA main loop (gemm_tile.h) and folds each tile into a
// register-resident key per (row, lane): c = acc * inv_e * inv_f / max(|e| |f_g|, 1e-8), r = relu(c), key (r, raster index
// y * gw + x), separator columns (x >= gw) skipped.  acc[i][j][r] of wave (wm, wn) is row wm*64 + 16 i + 4 (lane >> 4) + r,
// column tn*128 + wn*64 + 16 j + (lane & 15).  The 16 lanes of a row and the two column waves combine once at the end.
// Phase 2, one wave per row: the cells of the disc dx^2 + dy^2 <= radius^2 (pixels) around the argmax cell are scored again
// in fp32 from the fp32 (or input) features — four cells at a time, 16 lanes each — and p = sum xy(g) exp(r_g) / sum exp(r_g).
// ---------------------------------------------------------------------------------------------------------------------
template <typename T, typename S>
__global__ __launch_bounds__(256) void track_points_kernel(const T* E, const T* F, const S* Es, const S* Fs, const float* enorm,
                                                           const float* fnorm, const float* inv_e, const float* inv_f,
                                                           const int4* tiles, int gh, int gw, int pitch, int D, int half_patch,
                                                           int stride, int radius, int rc, float* xy, int* cell) {
    __shared__ __attribute__((aligned(16))) char smem[GD_TILE_SMEM];
    const int4 tl = tiles[blockIdx.x];
    const int frame = tl.x, row0 = tl.y, nrows = tl.z, out0 = tl.w;
    const int ncell = gh * pitch;
    const long ld = (long)D * sizeof(T);
    const char* Eb = (const char*)(E + (long)row0 * D);
    const char* Fb = (const char*)(F + (long)frame * ncell * D);
    const float* fn = fnorm + (long)frame * ncell;
    const float sc = (inv_e ? *inv_e : 1.f) * (inv_f ? *inv_f : 1.f);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
    const int rl0 = wm * 64 + 4 * (lane >> 4), cl0 = wn * 64 + (lane & 15);
    float en[4][4];
    unsigned long long best[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = rl0 + 16 * i + r;
            en[i][r] = row < nrows ? enorm[row0 + row] : 1.f;
            best[i][r] = 0;
        }
    const int nt = (ncell + 127) / 128;
    for (int tn = 0; tn < nt; ++tn) {
        f32x4 acc[4][4];
        mma_tile_128x128<T>(Eb, ld, nrows, Fb, ld, ncell, (int)ld, 0, tn, smem, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = tn * 128 + cl0 + 16 * j;
            const int y = c / pitch, x = c - y * pitch;
            if (c < ncell && x < gw) {
                const float nf = fn[c];
                const int g = y * gw + x;
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = acc[i][j][r] * sc / fmaxf(en[i][r] * nf, 1e-8f);
                        best[i][r] = umax64(best[i][r], gd_key(v > 0.f ? v : 0.f, g));
                    }
            }
        }
    }
    unsigned long long* srow = (unsigned long long*)smem;    // [wn][128]: the main loop ended on a barrier, smem is free
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const unsigned long long b = row16_max_u64(best[i][r]);
            if ((lane & 15) == 0) srow[wn * 128 + rl0 + 16 * i + r] = b;
        }
    __syncthreads();

    const int grp = lane >> 4, l16 = lane & 15, side = 2 * rc + 1;
    for (int row = wave; row < nrows; row += 4) {
        const int gs = gd_key_index(umax64(srow[row], srow[128 + row]));
        const int cy = gs / gw, cx = gs - cy * gw;
        const S* e = Es + (long)(row0 + row) * D;
        const float ne = enorm[row0 + row];
        const S* fb = Fs + (long)frame * ncell * D;
        float sw = 0.f, sx = 0.f, sy = 0.f;
        for (int q = grp; q < side * side; q += 4) {
            const int dy = q / side - rc, dx = q - (q / side) * side - rc;
            const int yy = cy + dy, xx = cx + dx;
            if ((dx * stride) * (dx * stride) + (dy * stride) * (dy * stride) > radius * radius || yy < 0 || yy >= gh || xx < 0 ||
                xx >= gw)
                continue;                                    // uniform over the 16 lanes of the group
            const long cm = (long)yy * pitch + xx;
            const S* f = fb + cm * D;
            float d = 0.f;
            for (int k = 4 * l16; k < D; k += 64) {
                const f32x4 a = load4_f32(e + k), b = load4_f32(f + k);
                d = fmaf(a[0], b[0], d);
                d = fmaf(a[1], b[1], d);
                d = fmaf(a[2], b[2], d);
                d = fmaf(a[3], b[3], d);
            }
            d += __shfl_xor(d, 8, 64);
            d += __shfl_xor(d, 4, 64);
            d += __shfl_xor(d, 2, 64);
            d += __shfl_xor(d, 1, 64);
            const float c = d / fmaxf(ne * fn[cm], 1e-8f);
            const float w = expf(c > 0.f ? c : 0.f);
            sw += w;
            sx += w * (float)(xx * stride + half_patch);
            sy += w * (float)(yy * stride + half_patch);
        }
        // the four groups' partial sums (every lane of a group holds the same values)
        sw += __shfl_xor(sw, 16, 64);
        sx += __shfl_xor(sx, 16, 64);
        sy += __shfl_xor(sy, 16, 64);
        sw += __shfl_xor(sw, 32, 64);
        sx += __shfl_xor(sx, 32, 64);
        sy += __shfl_xor(sy, 32, 64);
        if (lane == 0) {
            const long o = (long)out0 + row;
            xy[2 * o] = sx / sw;
            xy[2 * o + 1] = sy / sw;
            if (cell) cell[o] = gs;
        }
    }
}

static size_t gd_align256(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" int gd_track_row_norms(const void* X, long rows, int D, int dtype, float* norms, void* stream) {
    GD_REQUIRE(X && norms, "gd_track_row_norms: X and norms are required");
    GD_REQUIRE(rows > 0 && D > 0, "gd_track_row_norms: need rows, D > 0 (rows=%ld D=%d)", rows, D);
    GD_REQUIRE(dtype == GD_F32 || dtype == GD_F16 || dtype == GD_BF16, "gd_track_row_norms: bad dtype %d", dtype);
    GD_REQUIRE((rows + 3) / 4 < (1L << 31), "gd_track_row_norms: %ld rows exceed the grid", rows);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((rows + 3) / 4));
    if (dtype == GD_F32)
        hipLaunchKernelGGL(track_row_norms_kernel<float>, grid, dim3(256), 0, s, (const float*)X, rows, D, norms);
    else if (dtype == GD_F16)
        hipLaunchKernelGGL(track_row_norms_kernel<f16>, grid, dim3(256), 0, s, (const f16*)X, rows, D, norms);
    else
        hipLaunchKernelGGL(track_row_norms_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)X, rows, D, norms);
    GD_LAUNCH_OK();
    return 0;
}

extern "C" size_t gd_track_points_workspace_bytes(int n_tiles) { return n_tiles > 0 ? gd_align256((size_t)n_tiles * 16) : 0; }

template <typename T, typename S>
static void track_launch(int n_tiles, hipStream_t s, const void* E, const void* F, const void* Es, const void* Fs, const float* e_norm,
                         const float* f_norm, const float* inv_e, const float* inv_f, const int4* tiles, int gh, int gw, int pitch, int D,
                         int patch, int stride, int radius, float* xy, int* cell) {
    hipLaunchKernelGGL((track_points_kernel<T, S>), dim3(n_tiles), dim3(256), 0, s, (const T*)E, (const T*)F, (const S*)Es, (const S*)Fs,
                       e_norm, f_norm, inv_e, inv_f, tiles, gh, gw, pitch, D, patch / 2, stride, radius, (radius + stride - 1) / stride, xy,
                       cell);
}

extern "C" int gd_track_points(const void* E, const void* F, const void* E_src, const void* F_src, int dtype, int src_dtype, long E_rows,
                               int T, int gh, int gw, int pitch, int D, int img_h, int img_w, int patch, int stride, int radius,
                               const float* e_norm, const float* f_norm, const float* inv_scale_e, const float* inv_scale_f,
                               const int* tiles, int n_tiles, long n_out, float* xy, int* cell, void* workspace, void* stream) {
    GD_REQUIRE(E && F && E_src && F_src && e_norm && f_norm && tiles && xy && workspace,
               "gd_track_points: E, F, E_src, F_src, e_norm, f_norm, tiles, xy and workspace are required");
    GD_REQUIRE(dtype == GD_F32 || dtype == GD_F16 || dtype == GD_BF16, "gd_track_points: bad operand dtype %d", dtype);
    GD_REQUIRE(src_dtype == GD_F32 || src_dtype == dtype,
               "gd_track_points: the recompute features are fp32 or the operand dtype (dtype %d, src_dtype %d)", dtype, src_dtype);
    GD_REQUIRE(dtype != GD_F32 || (E_src == E && F_src == F), "gd_track_points: fp32 operands are their own recompute features");
    GD_REQUIRE(D > 0 && D % 8 == 0, "gd_track_points: D must be a positive multiple of 8 (D=%d)", D);
    GD_REQUIRE(T > 0 && E_rows > 0 && n_out > 0 && n_tiles > 0, "gd_track_points: need T, E_rows, n_out, n_tiles > 0 (T=%d E_rows=%ld n_out=%ld "
               "n_tiles=%d)", T, E_rows, n_out, n_tiles);
    GD_REQUIRE(patch > 0 && stride > 0 && radius >= 0 && img_h >= patch && img_w >= patch,
               "gd_track_points: bad geometry (image %dx%d patch %d stride %d radius %d)", img_h, img_w, patch, stride, radius);
    GD_REQUIRE(gh == 1 + (img_h - patch) / stride && gw == 1 + (img_w - patch) / stride,
               "gd_track_points: grid %dx%d is not 1 + (image - patch) // stride for image %dx%d, patch %d, stride %d", gh, gw, img_h, img_w,
               patch, stride);
    GD_REQUIRE(pitch >= gw, "gd_track_points: pitch %d < gw %d", pitch, gw);
    GD_REQUIRE((long)gh * pitch < (1L << 31) && (long)T * gh * pitch < (1L << 31), "gd_track_points: %d frames of %dx%d cells exceed 2^31",
               T, gh, pitch);
    GD_REQUIRE(E_rows < (1L << 31) && n_out < (1L << 31), "gd_track_points: E_rows %ld / n_out %ld exceed 2^31", E_rows, n_out);
    GD_REQUIRE((long)radius * radius < (1L << 30), "gd_track_points: radius %d too large", radius);
    GD_REQUIRE(((uintptr_t)E & 15) == 0 && ((uintptr_t)F & 15) == 0 && ((uintptr_t)E_src & 15) == 0 && ((uintptr_t)F_src & 15) == 0,
               "gd_track_points: E, F, E_src and F_src must be 16-byte aligned");
    for (int t = 0; t < n_tiles; ++t) {
        const int fr = tiles[4 * t], r0 = tiles[4 * t + 1], nr = tiles[4 * t + 2], o0 = tiles[4 * t + 3];
        GD_REQUIRE(fr >= 0 && fr < T, "gd_track_points: tile %d: frame %d not in [0, %d)", t, fr, T);
        GD_REQUIRE(nr >= 1 && nr <= 128, "gd_track_points: tile %d: %d rows (1 to 128)", t, nr);
        GD_REQUIRE(r0 >= 0 && (long)r0 + nr <= E_rows, "gd_track_points: tile %d: rows [%d, %ld) outside E's %ld", t, r0, (long)r0 + nr, E_rows);
        GD_REQUIRE(o0 >= 0 && (long)o0 + nr <= n_out, "gd_track_points: tile %d: outputs [%d, %ld) outside %ld", t, o0, (long)o0 + nr, n_out);
    }
    hipStream_t s = (hipStream_t)stream;
    GD_REQUIRE(hipMemcpyAsync(workspace, tiles, (size_t)n_tiles * 16, hipMemcpyHostToDevice, s) == hipSuccess, "gd_track_points: tile copy failed");
    const int4* tl = (const int4*)workspace;
#define GD_TRACK_ARGS n_tiles, s, E, F, E_src, F_src, e_norm, f_norm, inv_scale_e, inv_scale_f, tl, gh, gw, pitch, D, patch, stride, radius, xy, cell
    if (dtype == GD_F32)
        track_launch<float, float>(GD_TRACK_ARGS);
    else if (dtype == GD_F16)
        src_dtype == GD_F32 ? track_launch<f16, float>(GD_TRACK_ARGS) : track_launch<f16, f16>(GD_TRACK_ARGS);
    else
        src_dtype == GD_F32 ? track_launch<bf16, float>(GD_TRACK_ARGS) : track_launch<bf16, bf16>(GD_TRACK_ARGS);
#undef GD_TRACK_ARGS
    GD_LAUNCH_OK();
    return 0;
}
