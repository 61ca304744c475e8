// The VGGT teacher's tracker tail (vggt/heads/track_modules/base_track_predictor.py:82-209 BaseTrackerPredictor.forward on
// blocks.py:147-246 CorrBlock and utils.py:18-226) without the correlation volume, the host-built position table and the layout
// round trips: pyramid pooling, fused correlation-window sampling, point sampling, the sampled position embedding and the two
// glue passes of an iteration.  Every map is channel-last [F, H, pitch, C] fp32 with C = 128; columns x >= W of a pitched row
// (the separator column of the fused DPT head's grids) are never read.
#include "gd_common.h"

#define VT_C 128                 // the only feature width served (latent_dim of the teacher's tracker)
#define VT_D (3 * VT_C + 4)      // the update transformer's input width: 388
#define VT_MAX_LEVELS 8
#define VT_MAX_RADIUS 4          // (2r + 2)^2 <= 128 cells per window

static bool vt_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------------------------------
// 2 x 2 mean, stride 2, floor sizes (F.avg_pool2d(kernel_size=2, stride=2), blocks.py:173): one thread per four channels of
// an output cell; separator columns of the output (x >= Wo) are written as zeros.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vt_avgpool2_kernel(const float* src, float* dst, int H, int W, int pitch_in, int Ho, int Wo,
                                                          int pitch_out, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % (VT_C / 4));
    long cell = i / (VT_C / 4);
    const int xo = (int)(cell % pitch_out);
    cell /= pitch_out;
    const int yo = (int)(cell % Ho);
    const long f = cell / Ho;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (xo < Wo) {
        const float* p = src + (((f * H + 2 * yo) * pitch_in + 2 * xo) * VT_C + 4 * c4);
        const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + VT_C);
        const f32x4 c = *(const f32x4*)(p + (long)pitch_in * VT_C), d = *(const f32x4*)(p + (long)pitch_in * VT_C + VT_C);
        v = ((a + b) + (c + d)) * 0.25f;
    }
    *(f32x4*)(dst + (((f * Ho + yo) * pitch_out + xo) * VT_C + 4 * c4)) = v;
}

// ---------------------------------------------------------------------------------------------------------------------
// Correlation-window sampling.  One wave per (frame, point, level): the target vector sits in registers (lane l holds channels
// 8 (l & 15) .. + 7), the four 16-lane groups each take every fourth cell of the (2r + 2)^2 integer window around
// coords / 2^level, and the window's dot products go to LDS for the shared-fraction blend.  Work items run frame-major and a
// contiguous range of them goes to one XCD, so the map rows neighbouring points share stay in that XCD's L2.
// ---------------------------------------------------------------------------------------------------------------------
struct VtLevels {
    const float* map[VT_MAX_LEVELS];
    int H[VT_MAX_LEVELS], W[VT_MAX_LEVELS], pitch[VT_MAX_LEVELS];
};

__global__ __launch_bounds__(256) void vt_corr_sample_kernel(VtLevels lv, const float* tgt, const float* coords, int S, int N, int L,
                                                             int r, int ld, float* out, long items) {
    __shared__ float dots[4][128];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane >> 4, l16 = lane & 15;
    const long item = (long)xcd_remap(blockIdx.x, gridDim.x) * 4 + wave;
    const bool live = item < items;
    const int side = 2 * r + 2, win = 2 * r + 1;
    int l = 0, f = 0, n = 0;
    float fx = 0.f, fy = 0.f;
    if (live) {
        l = (int)(item % L);
        const long fn = item / L;
        n = (int)(fn % N);
        f = (int)(fn / N);
        const int b = f / S, s = f - b * S;
        const long row = ((long)b * N + n) * S + s;                 // targets and coords are [B, N, S, .]
        const float* t = tgt + row * VT_C + 8 * l16;
        const f32x4 t0 = *(const f32x4*)t, t1 = *(const f32x4*)(t + 4);
        const float sc = 1.f / (float)(1 << l);                     // a power of two: the product is the reference's quotient
        const float x = coords[2 * row] * sc, y = coords[2 * row + 1] * sc;
        const int H = lv.H[l], W = lv.W[l], pitch = lv.pitch[l];
        int x0 = -(1 << 20), y0 = -(1 << 20);                       // a point no finite window reaches: every cell counts 0
        if (fabsf(x) < 1e9f && fabsf(y) < 1e9f) {                   // (false for NaN)
            const float xf = floorf(x), yf = floorf(y);
            x0 = (int)xf; y0 = (int)yf;
            fx = x - xf; fy = y - yf;                               // exact
        }
        const float* base = lv.map[l] + (long)f * H * pitch * VT_C + 8 * l16;
#pragma unroll 5
        for (int q = grp; q < side * side; q += 4) {
            const int i = q / side, j = q - i * side;
            const int iy = y0 - r + i, ix = x0 - r + j;
            const bool in = ix >= 0 && ix < W && iy >= 0 && iy < H;
            // the load itself is unconditional, from a clamped (valid) cell, so that several are in flight per lane
            const int cy = min(max(iy, 0), H - 1), cx = min(max(ix, 0), W - 1);
            const float* p = base + ((long)cy * pitch + cx) * VT_C;
            const f32x4 a0 = *(const f32x4*)p, a1 = *(const f32x4*)(p + 4);
            float d = t0[0] * a0[0];
            d = fmaf(t0[1], a0[1], d);
            d = fmaf(t0[2], a0[2], d);
            d = fmaf(t0[3], a0[3], d);
            d = fmaf(t1[0], a1[0], d);
            d = fmaf(t1[1], a1[1], d);
            d = fmaf(t1[2], a1[2], d);
            d = fmaf(t1[3], a1[3], d);
            d = row16_sum(d);
            if (l16 == 0) dots[wave][q] = in ? d * 0.08838834764831845f : 0.f;      // 1 / sqrt(128)
        }
    }
    __syncthreads();
    if (!live) return;
    float* o = out + ((long)f * N + n) * ld;
    const float* D = dots[wave];
    for (int k = lane; k < win * win; k += 64) {
        // the reference's window is transposed (blocks.py:181-184 stacks meshgrid(dy, dx, "ij") onto an (x, y) centroid):
        // entry a * (2r+1) + b is the sample at (x + a - r, y + b - r)
        const int a = k / win, b = k - a * win;
        const float d00 = D[b * side + a], d01 = D[b * side + a + 1], d10 = D[(b + 1) * side + a], d11 = D[(b + 1) * side + a + 1];
        o[(long)l * win * win + k] = (1.f - fy) * ((1.f - fx) * d00 + fx * d01) + fy * ((1.f - fx) * d10 + fx * d11);
    }
    if (l == 0)
        for (int k = L * win * win + lane; k < ld; k += 64) o[k] = 0.f;            // the GEMM's padded K
}

// ---------------------------------------------------------------------------------------------------------------------
// Bilinear sample of a channel-last map at N points per batch entry, align_corners=True, border padding (utils.py:196-226
// sample_features4d on bilinear_sampler's defaults): one thread per four channels of a point.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vt_points_bilinear_kernel(const float* map, const float* pts, float* out, int N, int H, int W,
                                                                 int pitch, long frame_step, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % (VT_C / 4));
    const long pt = i / (VT_C / 4), b = pt / N;
    const float x = fminf(fmaxf(pts[2 * pt], 0.f), (float)(W - 1)), y = fminf(fmaxf(pts[2 * pt + 1], 0.f), (float)(H - 1));
    const float xf = floorf(x), yf = floorf(y), fx = x - xf, fy = y - yf;
    int x0 = (int)xf, y0 = (int)yf;
    x0 = min(max(x0, 0), W - 1); y0 = min(max(y0, 0), H - 1);                      // (a NaN coordinate lands on cell 0)
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float* m = map + b * frame_step * H * pitch * VT_C + 4 * c4;
    const f32x4 v00 = *(const f32x4*)(m + ((long)y0 * pitch + x0) * VT_C), v01 = *(const f32x4*)(m + ((long)y0 * pitch + x1) * VT_C);
    const f32x4 v10 = *(const f32x4*)(m + ((long)y1 * pitch + x0) * VT_C), v11 = *(const f32x4*)(m + ((long)y1 * pitch + x1) * VT_C);
    *(f32x4*)(out + pt * VT_C + 4 * c4) = (1.f - fy) * ((1.f - fx) * v00 + fx * v01) + fy * ((1.f - fx) * v10 + fx * v11);
}

// ---------------------------------------------------------------------------------------------------------------------
// The 2-D sin/cos position table (utils.py:18-90) sampled at M points (base_track_predictor.py:149-150).  The table is
// separable — channels [0, D/2) are [sin | cos](x w_k), channels [D/2, D) the same of y — so the bilinear sample with border
// clamp is a 1-D blend of two columns per half.  One thread per (point, k): four outputs.  Full-range sinf / cosf.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vt_pos_embed_kernel(const float* pts, const float* omega, float* out, int H, int W, int D, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int q = D / 4, k = (int)(i % q);
    const long pt = i / q;
    const float w = omega[k];
    float* o = out + pt * D;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = h ? H : W;
        const float v = fminf(fmaxf(pts[2 * pt + h], 0.f), (float)(n - 1));
        const float vf = floorf(v), fr = v - vf;
        const float p0 = fminf(fmaxf(vf, 0.f), (float)(n - 1)), p1 = fminf(p0 + 1.f, (float)(n - 1));
        const float a0 = p0 * w, a1 = p1 * w;
        o[h * 2 * q + k] = (1.f - fr) * sinf(a0) + fr * sinf(a1);
        o[h * 2 * q + q + k] = (1.f - fr) * cosf(a0) + fr * cosf(a1);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Input assembly of one iteration (base_track_predictor.py:135-160), rows (b, n, s): one thread per four of the 388 channels.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vt_assemble_kernel(const float* coords, const float* corr, const float* feats, const float* pos,
                                                          const float* qrt, float* x, int S, int N, float max_scale, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % (VT_D / 4));
    const long row = i / (VT_D / 4);                    // (b * N + n) * S + s
    const int s = (int)(row % S);
    const long bn = row / S, b = bn / N, n = bn - b * N;
    const float flx = coords[2 * row] - coords[2 * (row - s)], fly = coords[2 * row + 1] - coords[2 * (row - s) + 1];
    f32x4 v;
    if (c4 < VT_C / 4) {
        // get_2d_embedding(flows, 64, cat_coords=False) (utils.py:93-124): [x: sin, cos interleaved (64) | y: the same (64)],
        // arguments flow * (2k * 1000 / 64) formed in fp32 as the reference forms them
        const int c = 4 * c4, cc = c & (VT_C / 2 - 1), k = cc >> 1;
        const float fl = c < VT_C / 2 ? flx : fly;
        const float a0 = fl * ((float)(2 * k) * (1000.0f / (VT_C / 2))), a1 = fl * ((float)(2 * k + 2) * (1000.0f / (VT_C / 2)));
        v = f32x4{sinf(a0), cosf(a0), sinf(a1), cosf(a1)};
    } else if (c4 == VT_C / 4) {
        v = f32x4{flx / max_scale, fly / max_scale, flx / max_scale, fly / max_scale};
    } else if (c4 < VT_C / 2 + 1) {
        v = *(const f32x4*)(corr + ((b * S + s) * N + n) * VT_C + 4 * (c4 - VT_C / 4 - 1));       // corr_mlp's rows are (b, s, n)
    } else {
        v = *(const f32x4*)(feats + row * VT_C + 4 * (c4 - VT_C / 2 - 1));
    }
    const f32x4 p = *(const f32x4*)(pos + bn * VT_D + 4 * c4), t = *(const f32x4*)(qrt + (s > 0 ? VT_D : 0) + 4 * c4);
    *(f32x4*)(x + row * VT_D + 4 * c4) = (v + p) + t;
}

// ---------------------------------------------------------------------------------------------------------------------
// Update of one iteration (base_track_predictor.py:169-192), rows (b, n, s): coords += delta[:2] with frame 0 pinned to the
// query, the prediction at image scale written as [B, S, N, 2], and delta[2:] copied to aligned rows for the feature update.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void vt_update_kernel(const float* delta, long ldd, float* coords, float* pred, float* dfeat, int S, int N,
                                                        float mul1, float mul2, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % (VT_C / 4 + 1));
    const long row = i / (VT_C / 4 + 1);
    const float* d = delta + row * ldd;
    if (c4 < VT_C / 4) {
        *(f32x4*)(dfeat + row * VT_C + 4 * c4) = f32x4{d[2 + 4 * c4], d[3 + 4 * c4], d[4 + 4 * c4], d[5 + 4 * c4]};
        return;
    }
    const int s = (int)(row % S);
    const long bn = row / S, b = bn / N, n = bn - b * N;
    float cx = coords[2 * row], cy = coords[2 * row + 1];
    if (s > 0) {
        cx += d[0]; cy += d[1];
        coords[2 * row] = cx; coords[2 * row + 1] = cy;
    }
    float* p = pred + 2 * ((b * S + s) * N + n);
    p[0] = (cx * mul1) * mul2;
    p[1] = (cy * mul1) * mul2;
}

// =====================================================================================================================
extern "C" int gd_avgpool2_cl(const float* src, float* dst, int frames, int H, int W, int pitch_in, int pitch_out, int C, void* stream) {
    GD_REQUIRE(C == VT_C, "gd_avgpool2_cl: C = %d: the tracker kernels serve C = %d only", C, VT_C);
    GD_REQUIRE(frames > 0 && H >= 2 && W >= 2, "gd_avgpool2_cl: need frames > 0 and a map of at least 2 x 2 (frames=%d H=%d W=%d)", frames, H, W);
    GD_REQUIRE(pitch_in >= W && pitch_out >= W / 2, "gd_avgpool2_cl: pitch_in %d < W %d or pitch_out %d < W / 2 = %d", pitch_in, W, pitch_out, W / 2);
    GD_REQUIRE(src && dst && vt_aligned16(src) && vt_aligned16(dst), "gd_avgpool2_cl: src and dst are required, 16-byte aligned");
    const long total = (long)frames * (H / 2) * pitch_out * (VT_C / 4);
    GD_REQUIRE((total + 255) / 256 < (1L << 31), "gd_avgpool2_cl: %ld work items exceed the grid", total);
    hipLaunchKernelGGL(vt_avgpool2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, H, W, pitch_in, H / 2,
                       W / 2, pitch_out, total);
    GD_LAUNCH_OK();
    return 0;
}

extern "C" int gd_corr_sample(const float* const* maps, const int* dims, int levels, int radius, const float* targets, const float* coords,
                              int B, int S, int N, int C, float* out, long ld, void* stream) {
    GD_REQUIRE(C == VT_C, "gd_corr_sample: C = %d: the tracker kernels serve C = %d only", C, VT_C);
    GD_REQUIRE(levels >= 1 && levels <= VT_MAX_LEVELS, "gd_corr_sample: %d levels (1 to %d)", levels, VT_MAX_LEVELS);
    GD_REQUIRE(radius >= 0 && radius <= VT_MAX_RADIUS, "gd_corr_sample: radius %d (0 to %d: (2r + 2)^2 <= 128 cells)", radius, VT_MAX_RADIUS);
    GD_REQUIRE(B > 0 && S > 0 && N > 0, "gd_corr_sample: need B, S, N > 0 (B=%d S=%d N=%d)", B, S, N);
    GD_REQUIRE(maps && dims && targets && coords && out, "gd_corr_sample: maps, dims, targets, coords and out are required");
    const int win = 2 * radius + 1;
    GD_REQUIRE(ld >= (long)levels * win * win, "gd_corr_sample: ld %ld < levels * (2r + 1)^2 = %d", ld, levels * win * win);
    GD_REQUIRE(ld < (1L << 31), "gd_corr_sample: ld %ld exceeds 2^31", ld);
    GD_REQUIRE(vt_aligned16(targets), "gd_corr_sample: targets must be 16-byte aligned");
    VtLevels lv;
    for (int l = 0; l < levels; ++l) {
        const int H = dims[3 * l], W = dims[3 * l + 1], pitch = dims[3 * l + 2];
        GD_REQUIRE(H >= 1 && W >= 1 && pitch >= W, "gd_corr_sample: level %d: bad map %d x %d, pitch %d", l, H, W, pitch);
        // a side of 1: the reference's 2 / max(size - 1, 1) normalisation sends every sample to cell 0 there, which this form does not reproduce
        GD_REQUIRE(H >= 2 && W >= 2, "gd_corr_sample: level %d is %d x %d: a level with a side of 1 is not served (use fewer levels or a larger map)",
                   l, H, W);
        GD_REQUIRE((long)B * S * H * pitch < (1L << 31), "gd_corr_sample: level %d: %d frames of %d x %d cells exceed 2^31", l, B * S, H, pitch);
        GD_REQUIRE(maps[l] && vt_aligned16(maps[l]), "gd_corr_sample: level %d: the map is required, 16-byte aligned", l);
        lv.map[l] = maps[l]; lv.H[l] = H; lv.W[l] = W; lv.pitch[l] = pitch;
    }
    for (int l = levels; l < VT_MAX_LEVELS; ++l) { lv.map[l] = nullptr; lv.H[l] = lv.W[l] = lv.pitch[l] = 0; }
    const long items = (long)B * S * N * levels;
    GD_REQUIRE((items + 3) / 4 < (1L << 31), "gd_corr_sample: %ld work items exceed the grid", items);
    hipLaunchKernelGGL(vt_corr_sample_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, (hipStream_t)stream, lv, targets, coords, S, N, levels,
                       radius, (int)ld, out, items);
    GD_LAUNCH_OK();
    return 0;
}

extern "C" int gd_points_bilinear(const float* map, const float* points, float* out, int B, int N, int H, int W, int pitch, int C, long frame_step,
                                  void* stream) {
    GD_REQUIRE(C == VT_C, "gd_points_bilinear: C = %d: the tracker kernels serve C = %d only", C, VT_C);
    GD_REQUIRE(B > 0 && N > 0 && H >= 1 && W >= 1 && pitch >= W && frame_step >= 1,
               "gd_points_bilinear: need B, N > 0, a map of at least 1 x 1, pitch >= W, frame_step >= 1 (B=%d N=%d H=%d W=%d pitch=%d frame_step=%ld)", B, N,
               H, W, pitch, frame_step);
    GD_REQUIRE(map && points && out && vt_aligned16(map) && vt_aligned16(out), "gd_points_bilinear: map, points and out are required; map and out 16-byte aligned");
    const long total = (long)B * N * (VT_C / 4);
    GD_REQUIRE((total + 255) / 256 < (1L << 31), "gd_points_bilinear: %ld work items exceed the grid", total);
    hipLaunchKernelGGL(vt_points_bilinear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, map, points, out, N, H, W,
                       pitch, frame_step, total);
    GD_LAUNCH_OK();
    return 0;
}

extern "C" int gd_track_pos_embed(const float* points, const float* omega, float* out, long M, int H, int W, int D, void* stream) {
    GD_REQUIRE(D > 0 && D % 4 == 0, "gd_track_pos_embed: D = %d must be a positive multiple of 4", D);
    GD_REQUIRE(M > 0 && H >= 1 && W >= 1, "gd_track_pos_embed: need M > 0 and a grid of at least 1 x 1 (M=%ld H=%d W=%d)", M, H, W);
    GD_REQUIRE(H < (1 << 24) && W < (1 << 24), "gd_track_pos_embed: grid %d x %d: indices must be exact in fp32", H, W);
    GD_REQUIRE(points && omega && out, "gd_track_pos_embed: points, omega and out are required");
    const long total = M * (D / 4);
    GD_REQUIRE((total + 255) / 256 < (1L << 31), "gd_track_pos_embed: %ld work items exceed the grid", total);
    hipLaunchKernelGGL(vt_pos_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, points, omega, out, H, W, D, total);
    GD_LAUNCH_OK();
    return 0;
}

extern "C" int gd_track_assemble(const float* coords, const float* corr, const float* feats, const float* pos, const float* ref_token, float* x,
                                 int B, int S, int N, int C, float max_scale, void* stream) {
    GD_REQUIRE(C == VT_C, "gd_track_assemble: C = %d: the tracker kernels serve C = %d only", C, VT_C);
    GD_REQUIRE(B > 0 && S > 0 && N > 0, "gd_track_assemble: need B, S, N > 0 (B=%d S=%d N=%d)", B, S, N);
    GD_REQUIRE(max_scale != 0.f, "gd_track_assemble: max_scale must not be 0");
    GD_REQUIRE(coords && corr && feats && pos && ref_token && x, "gd_track_assemble: coords, corr, feats, pos, ref_token and x are required");
    GD_REQUIRE(vt_aligned16(corr) && vt_aligned16(feats) && vt_aligned16(pos) && vt_aligned16(ref_token) && vt_aligned16(x),
               "gd_track_assemble: corr, feats, pos, ref_token and x must be 16-byte aligned");
    const long total = (long)B * N * S * (VT_D / 4);
    GD_REQUIRE((total + 255) / 256 < (1L << 31), "gd_track_assemble: %ld work items exceed the grid", total);
    hipLaunchKernelGGL(vt_assemble_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, coords, corr, feats, pos, ref_token,
                       x, S, N, max_scale, total);
    GD_LAUNCH_OK();
    return 0;
}

extern "C" int gd_track_update(const float* delta, long ldd, float* coords, float* pred, float* dfeat, int B, int S, int N, int C, float mul1,
                               float mul2, void* stream) {
    GD_REQUIRE(C == VT_C, "gd_track_update: C = %d: the tracker kernels serve C = %d only", C, VT_C);
    GD_REQUIRE(B > 0 && S > 0 && N > 0, "gd_track_update: need B, S, N > 0 (B=%d S=%d N=%d)", B, S, N);
    GD_REQUIRE(ldd >= VT_C + 2, "gd_track_update: ldd %ld < C + 2 = %d", ldd, VT_C + 2);
    GD_REQUIRE(delta && coords && pred && dfeat && vt_aligned16(dfeat), "gd_track_update: delta, coords, pred and dfeat are required; dfeat 16-byte aligned");
    const long total = (long)B * N * S * (VT_C / 4 + 1);
    GD_REQUIRE((total + 255) / 256 < (1L << 31), "gd_track_update: %ld work items exceed the grid", total);
    hipLaunchKernelGGL(vt_update_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, delta, ldd, coords, pred, dfeat, S, N,
                       mul1, mul2, total);
    GD_LAUNCH_OK();
    return 0;
}
