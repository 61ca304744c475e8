// The spatial glue of a DPT dense-prediction head (vggt/heads/dpt_head.py; the CroCo adapter of mast3r/catmlp_dpt_head.py) around gd_gemm_nt: every grid
// is channel-last on the separator-column layout of gd_stack3_rows, [frames, gh * (gw + 1), C], so that each 3x3 convolution of the head is one GEMM on
// the overlapping-row view of a 3-row stacked operand.  All five kernels are bandwidth kernels with 16-byte accesses and grid-stride loops: one output
// chunk per thread, except gd_mast3r_head_out, where sixteen lanes share a pixel.
#include "gd_common.h"

static inline int dpt_blocks(long total) { long b = (total + 255) / 256; return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b)); }

// N consecutive channels (N = 4 | 8) of a f32 | bf16 row as floats, by 16-byte (8-byte: four bf16) loads
template <typename TS, int N> __device__ __forceinline__ void dpt_load(const TS* p, float (&v)[N]);
template <> __device__ __forceinline__ void dpt_load<float, 4>(const float* p, float (&v)[4]) {
    const f32x4 a = *(const f32x4*)p;
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
}
template <> __device__ __forceinline__ void dpt_load<float, 8>(const float* p, float (&v)[8]) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
    v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
}
template <> __device__ __forceinline__ void dpt_load<bf16, 4>(const bf16* p, float (&v)[4]) {
    const bf16x4 a = *(const bf16x4*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (float)a[k];
}
template <> __device__ __forceinline__ void dpt_load<bf16, 8>(const bf16* p, float (&v)[8]) {
    const bf16x8 a = *(const bf16x8*)p;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (float)a[k];
}
template <typename TD, int N> __device__ __forceinline__ void dpt_store(TD* p, const float (&v)[N]) {
    static_assert(N * sizeof(TD) == 16, "one 16-byte store");
    alignas(16) TD o[N];
#pragma unroll
    for (int k = 0; k < N; ++k) o[k] = from_f32<TD>(v[k]);
    *(uint4*)p = *(const uint4*)o;
}

// ---- gd_grid_resample ---------------------------------------------------------------------------------------------------------------
// One output pixel (b, y, x), channels [c, c + N): the source sample (bilinear align_corners=True, or source pixel (y * step, x * step) for
// step >= 1), + addend, + the separable position tables, ReLU last.  The bilinear source coordinate y (sh - 1) / (dh - 1) is split into its
// integer part and remainder in integer arithmetic: one rounding (of the remainder's quotient), whatever the size.
struct ResampleArgs {
    int frames, sh, sw, dh, dw, C, step, relu;
    const float* addend;
    const float* px;
    const float* py;
};
template <typename TS, int N>
__device__ __forceinline__ void resample_pixel(const TS* src, const ResampleArgs& a, int b, int y, int x, int c, float (&v)[N]) {
    const long sp = a.sw + 1;
    const TS* s = src + (long)b * a.sh * sp * a.C + c;
    if (a.step >= 1) {
        dpt_load<TS, N>(s + ((long)y * a.step * sp + (long)x * a.step) * a.C, v);
    } else {
        const int ny = y * (a.sh - 1), dy = a.dh > 1 ? a.dh - 1 : 1, nx = x * (a.sw - 1), dx = a.dw > 1 ? a.dw - 1 : 1;
        const int y0 = ny / dy, x0 = nx / dx, y1 = min(y0 + 1, a.sh - 1), x1 = min(x0 + 1, a.sw - 1);
        const float fy = (float)(ny - y0 * dy) / (float)dy, fx = (float)(nx - x0 * dx) / (float)dx;
        float v00[N], v01[N], v10[N], v11[N];
        dpt_load<TS, N>(s + ((long)y0 * sp + x0) * a.C, v00);
        dpt_load<TS, N>(s + ((long)y0 * sp + x1) * a.C, v01);
        dpt_load<TS, N>(s + ((long)y1 * sp + x0) * a.C, v10);
        dpt_load<TS, N>(s + ((long)y1 * sp + x1) * a.C, v11);
#pragma unroll
        for (int k = 0; k < N; ++k)
            v[k] = (1.0f - fy) * ((1.0f - fx) * v00[k] + fx * v01[k]) + fy * ((1.0f - fx) * v10[k] + fx * v11[k]);
    }
    if (a.addend) {
        float t[N];
        dpt_load<float, N>(a.addend + (((long)b * a.dh + y) * (a.dw + 1) + x) * a.C + c, t);
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += t[k];
    }
    if (a.px) {
        const int C2 = a.C / 2;                       // C % 8 == 0: a group of four channels lies in one half
#pragma unroll
        for (int g = 0; g < N; g += 4) {
            const int cc = c + g;
            float t[4];
            dpt_load<float, 4>(cc < C2 ? a.px + (long)x * C2 + cc : a.py + (long)y * C2 + cc - C2, t);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[g + k] += t[k];
        }
    }
    if (a.relu) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = v[k] < 0.f ? 0.f : v[k];      // (a NaN stays a NaN)
    }
}

// STACK = false: dst the pitched grid [frames * dh * (dw + 1), C] (separators zero);  true: the operand of gd_stack3_rows,
// [frames * dh * (dw + 1) + 2, 3 C]: row R = r + 1 holds the pixels above, at and below r (zeros outside the image, at separators and in the guard rows)
template <typename TS, typename TD, bool STACK>
__global__ __launch_bounds__(256) void grid_resample_kernel(const TS* src, TD* dst, ResampleArgs a) {
    constexpr int N = 16 / sizeof(TD);
    const int pitch = a.dw + 1, cpr = a.C / N, slots = STACK ? 3 : 1;
    const long grows = (long)a.frames * a.dh * pitch, total = (grows + (STACK ? 2 : 0)) * slots * cpr;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int ch = (int)(i % cpr);
        const long t = i / cpr;
        const int slot = STACK ? (int)(t % 3) : 1;
        const long r = STACK ? t / 3 - 1 : t;
        float v[N];
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = 0.f;
        if (r >= 0 && r < grows) {
            const int b = (int)(r / ((long)a.dh * pitch)), rem = (int)(r % ((long)a.dh * pitch));
            const int y = rem / pitch + slot - 1, x = rem % pitch;
            if (x < a.dw && y >= 0 && y < a.dh) resample_pixel<TS, N>(src, a, b, y, x, ch * N, v);
        }
        dpt_store<TD, N>(dst + i * N, v);
    }
}

extern "C" int gd_grid_resample(const void* src, int src_dtype, void* dst, int dst_dtype, int stacked, int frames, int sh, int sw, int dh, int dw,
                                int C, int step, const float* addend, const float* px, const float* py, int relu, void* stream) {
    GD_REQUIRE(frames > 0 && sh > 0 && sw > 0 && dh > 0 && dw > 0 && C > 0 && step >= 0,
               "gd_grid_resample: bad shape frames=%d %dx%d -> %dx%d C=%d step=%d", frames, sh, sw, dh, dw, C, step);
    GD_REQUIRE(C % 8 == 0, "gd_grid_resample: C = %d is not a multiple of 8 (16-byte chunks of either element type, four-channel table groups)", C);
    GD_REQUIRE(src_dtype == GD_F32 || src_dtype == GD_BF16, "gd_grid_resample: source dtype %d: f32 or bf16", src_dtype);
    GD_REQUIRE(dst_dtype == GD_F32 || (stacked && dst_dtype == GD_BF16), "gd_grid_resample: dst dtype %d: a pitched grid is f32, a stacked operand f32 or bf16", dst_dtype);
    GD_REQUIRE((px == nullptr) == (py == nullptr), "gd_grid_resample: px and py come together");
    GD_REQUIRE(step == 0 || ((long)(dh - 1) * step < sh && (long)(dw - 1) * step < sw),
               "gd_grid_resample: step %d: destination %dx%d reaches past the source %dx%d", step, dh, dw, sh, sw);
    GD_REQUIRE((long)frames * sh * (sw + 1) < (1L << 31) && (long)frames * dh * (dw + 1) + 2 < (1L << 31) && (long)sh * (dh > 1 ? dh - 1 : 1) < (1L << 31) &&
               (long)sw * (dw > 1 ? dw - 1 : 1) < (1L << 31), "gd_grid_resample: grid rows or coordinate products reach 2^31");
    GD_REQUIRE(src && dst && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0 && ((uintptr_t)addend & 15) == 0 && ((uintptr_t)px & 15) == 0 &&
               ((uintptr_t)py & 15) == 0, "gd_grid_resample: pointers must be 16-byte aligned (src, dst not null)");
    ResampleArgs a{frames, sh, sw, dh, dw, C, step, relu ? 1 : 0, addend, px, py};
    if (step == 0 && sh == dh && sw == dw) a.step = 1;            // the identity: a copy, bit for bit
    const int n = 16 / gd_dtype_size(dst_dtype);
    const long total = ((long)frames * dh * (dw + 1) + (stacked ? 2 : 0)) * (stacked ? 3 : 1) * (C / n);
    const dim3 g(dpt_blocks(total)), blk(256);
    hipStream_t s = (hipStream_t)stream;
#define GD_RESAMPLE(TS, TD, ST) hipLaunchKernelGGL((grid_resample_kernel<TS, TD, ST>), g, blk, 0, s, (const TS*)src, (TD*)dst, a)
    if (src_dtype == GD_F32) {
        if (!stacked) GD_RESAMPLE(float, float, false);
        else if (dst_dtype == GD_F32) GD_RESAMPLE(float, float, true);
        else GD_RESAMPLE(float, bf16, true);
    } else {
        if (!stacked) GD_RESAMPLE(bf16, float, false);
        else if (dst_dtype == GD_F32) GD_RESAMPLE(bf16, float, true);
        else GD_RESAMPLE(bf16, bf16, true);
    }
#undef GD_RESAMPLE
    GD_LAUNCH_OK();
    return 0;
}

// ---- gd_deconv_scatter --------------------------------------------------------------------------------------------------------------
// ConvTranspose2d with kernel = stride = k as a GEMM [rows, C_in] x [(ky, kx, n), C_in]^T and this pixel shuffle:
// dst(b, Y, X, n) = src[row (b, Y / k, X / k)][((Y % k) k + X % k) C_out + n] + bias[n] on the pitched grid (gh k) x (gw k), separators zero.
__global__ __launch_bounds__(256) void deconv_scatter_kernel(const float* src, const float* bias, float* dst, int frames, int gh, int gw, int src_pitch,
                                                             int k, int Cout) {
    const int cpr = Cout / 4, dh = gh * k, pitch = gw * k + 1;
    const long total = (long)frames * dh * pitch * cpr;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int n = (int)(i % cpr) * 4;
        const long r = i / cpr;
        const int b = (int)(r / ((long)dh * pitch)), rem = (int)(r % ((long)dh * pitch)), Y = rem / pitch, X = rem % pitch;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (X < gw * k) {
            float bv[4];
            dpt_load<float, 4>(src + (((long)b * gh + Y / k) * src_pitch + X / k) * ((long)k * k * Cout) + (long)((Y % k) * k + X % k) * Cout + n, v);
            dpt_load<float, 4>(bias + n, bv);
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] += bv[j];
        }
        dpt_store<float, 4>(dst + i * 4, v);
    }
}

extern "C" int gd_deconv_scatter(const float* src, const float* bias, float* dst, int frames, int gh, int gw, int src_pitch, int k, int Cout,
                                 void* stream) {
    GD_REQUIRE(frames > 0 && gh > 0 && gw > 0 && k >= 1 && k <= 8 && Cout > 0 && (src_pitch == gw || src_pitch == gw + 1),
               "gd_deconv_scatter: bad shape frames=%d grid %dx%d pitch %d k=%d C_out=%d", frames, gh, gw, src_pitch, k, Cout);
    GD_REQUIRE(Cout % 4 == 0, "gd_deconv_scatter: C_out = %d is not a multiple of 4", Cout);
    GD_REQUIRE((long)frames * gh * k * (gw * k + 1) < (1L << 31), "gd_deconv_scatter: destination rows reach 2^31");
    GD_REQUIRE(src && bias && dst && ((uintptr_t)src & 15) == 0 && ((uintptr_t)bias & 15) == 0 && ((uintptr_t)dst & 15) == 0,
               "gd_deconv_scatter: src, bias, dst must be 16-byte aligned and not null");
    const long total = (long)frames * gh * k * (gw * k + 1) * (Cout / 4);
    hipLaunchKernelGGL(deconv_scatter_kernel, dim3(dpt_blocks(total)), dim3(256), 0, (hipStream_t)stream, src, bias, dst, frames, gh, gw, src_pitch, k, Cout);
    GD_LAUNCH_OK();
    return 0;
}

// ---- gd_dpt_head_out ----------------------------------------------------------------------------------------------------------------
// The head's last layer, one thread per pixel: y = W x + b on the Cin rectified channels of the pitched map, values = act(y[:-1]),
// confidence = conf_act(y[-1]).  expf / expm1f, not the fast intrinsics: depth is exp of this value.
#define DPT_MAX_OUT 8
__device__ __forceinline__ float dpt_sigmoid(float y) { return 1.0f / (1.0f + expf(-y)); }
__global__ __launch_bounds__(256) void dpt_head_out_kernel(const float* x, const float* w, const float* bias, float* preds, float* conf, int frames, int H,
                                                           int W, int Cin, int od, int act, int conf_act) {
    const long total = (long)frames * H * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long fy = i / W;
        const float* row = x + (fy * (W + 1) + (i - fy * W)) * Cin;
        float y[DPT_MAX_OUT];
#pragma unroll
        for (int o = 0; o < DPT_MAX_OUT; ++o) y[o] = o < od ? bias[o] : 0.f;
        for (int c = 0; c < Cin; c += 4) {
            float v[4];
            dpt_load<float, 4>(row + c, v);
#pragma unroll
            for (int o = 0; o < DPT_MAX_OUT; ++o)
                if (o < od) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) y[o] = fmaf(v[k], w[o * Cin + c + k], y[o]);
                }
        }
#pragma unroll
        for (int o = 0; o < DPT_MAX_OUT; ++o) {
            if (o >= od) continue;
            const float t = y[o];
            if (o == od - 1) {
                conf[i] = conf_act == GD_DPT_CONF_EXPP1 ? 1.0f + expf(t) : conf_act == GD_DPT_CONF_EXPP0 ? expf(t) : conf_act == GD_DPT_CONF_SIGMOID ? dpt_sigmoid(t) : t;
            } else {
                float r = t;
                if (act == GD_DPT_ACT_EXP) r = expf(t);
                else if (act == GD_DPT_ACT_INV_LOG) r = copysignf(expm1f(fabsf(t)), t);
                else if (act == GD_DPT_ACT_RELU) r = t < 0.f ? 0.f : t;
                else if (act == GD_DPT_ACT_SIGMOID) r = dpt_sigmoid(t);
                preds[i * (od - 1) + o] = r;
            }
        }
    }
}

extern "C" int gd_dpt_head_out(const float* x, const float* w, const float* bias, float* preds, float* conf, int frames, int H, int W, int Cin,
                               int output_dim, int act, int conf_act, void* stream) {
    GD_REQUIRE(frames > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 4 == 0, "gd_dpt_head_out: bad shape frames=%d %dx%d C_in=%d (a multiple of 4)", frames, H, W, Cin);
    GD_REQUIRE(output_dim >= 2 && output_dim <= DPT_MAX_OUT, "gd_dpt_head_out: output_dim %d: served are 2 .. %d (values + one confidence)", output_dim, DPT_MAX_OUT);
    GD_REQUIRE(act >= GD_DPT_ACT_LINEAR && act <= GD_DPT_ACT_SIGMOID, "gd_dpt_head_out: unknown activation code %d", act);
    GD_REQUIRE(conf_act >= GD_DPT_CONF_EXPP1 && conf_act <= GD_DPT_CONF_LINEAR, "gd_dpt_head_out: unknown conf_activation code %d", conf_act);
    GD_REQUIRE((long)frames * H * (W + 1) < (1L << 31), "gd_dpt_head_out: pixel rows reach 2^31");
    GD_REQUIRE(x && w && bias && preds && conf && ((uintptr_t)x & 15) == 0, "gd_dpt_head_out: null pointer, or x not 16-byte aligned");
    hipLaunchKernelGGL(dpt_head_out_kernel, dim3(dpt_blocks((long)frames * H * W)), dim3(256), 0, (hipStream_t)stream, x, w, bias, preds, conf, frames, H, W,
                       Cin, output_dim, act, conf_act);
    GD_LAUNCH_OK();
    return 0;
}

// ---- gd_mast3r_head_out -------------------------------------------------------------------------------------------------------------
// The MASt3R head's last stage in one pass (mast3r/catmlp_dpt_head.py postprocess / forward, dust3r/heads/postprocess.py): the final 1x1
// convolution of the DPT adapter on the pitched rectified map, the pixel shuffle of the local-feature MLP's token rows (by addressing alone:
// lf columns are packed (i, j, c)), and every per-pixel activation.  MH_LANES lanes share one pixel: each takes 16-byte pieces of the Cin row
// (a wave's loads cover four whole contiguous rows), the od dot products and the descriptor's squared norm are reduced within the group by
// __shfl_xor (ds_bpermute: no LDS memory, and a handful of values per pixel beside the row stream), and the same lanes read and write the
// pixel's contiguous D + two_confs values.  expf / expm1f, not the fast intrinsics.
#define MH_LANES 16
#define MH_MAX_D 32
struct Mast3rHeadArgs {
    int frames, H, W, Cin, od, P, D, two_confs, pts_mode, conf_mode, desc_mode, dconf_mode;
    float conf_vmin, conf_vmax, dconf_vmin, dconf_vmax;
};
__device__ __forceinline__ float mh_group_sum(float v) {
#pragma unroll
    for (int m = MH_LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ float mh_conf(float y, int mode, float vmin, float vmax) {
    if (mode == GD_MH_CONF_EXP) {
        const float e = expf(y), lim = vmax - vmin;
        return vmin + (e > lim ? lim : e);                       // (a NaN stays a NaN, as torch's clip)
    }
    if (mode == GD_MH_CONF_SIGMOID) return (vmax - vmin) * dpt_sigmoid(y) + vmin;
    return y;
}
__global__ __launch_bounds__(256) void mast3r_head_out_kernel(const float* x, const float* w, const float* bias, const float* lf, float* pts3d, float* conf,
                                                              float* desc, float* desc_conf, Mast3rHeadArgs a) {
    constexpr int PPB = 256 / MH_LANES;                           // pixels per block and pass
    const int lane = threadIdx.x % MH_LANES, n = a.D + a.two_confs;
    const long total = (long)a.frames * a.H * a.W;
    for (long base = (long)blockIdx.x * PPB; base < total; base += (long)gridDim.x * PPB) {      // block-uniform trips: every lane reaches the shuffles
        const long p = base + threadIdx.x / MH_LANES;
        const bool valid = p < total;
        const long fy = valid ? p / a.W : 0;                      // frame * H + y
        const int px = valid ? (int)(p - fy * a.W) : 0;
        float y[4] = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
            const float* row = x + (fy * (a.W + 1) + px) * a.Cin;
            for (int c = lane * 4; c < a.Cin; c += MH_LANES * 4) {
                float v[4], wv[4];
                dpt_load<float, 4>(row + c, v);
#pragma unroll
                for (int o = 0; o < 4; ++o)
                    if (o < a.od) {
                        dpt_load<float, 4>(w + o * a.Cin + c, wv);
#pragma unroll
                        for (int k = 0; k < 4; ++k) y[o] = fmaf(v[k], wv[k], y[o]);
                    }
            }
        }
        // the pixel's D + two_confs <= 33 local-feature values: lane l holds elements l, l + MH_LANES and l + 2 MH_LANES
        float f0 = 0.f, f1 = 0.f, f2 = 0.f;
        if (valid && lf) {
            const int yy = (int)(fy % a.H), gh = a.H / a.P, gw = a.W / a.P;
            const long trow = ((fy / a.H) * gh + yy / a.P) * gw + px / a.P;
            const float* src = lf + trow * ((long)a.P * a.P * n) + (long)((yy % a.P) * a.P + px % a.P) * n;
            if (lane < n) f0 = src[lane];
            if (lane + MH_LANES < n) f1 = src[lane + MH_LANES];
            if (lane + 2 * MH_LANES < n) f2 = src[lane + 2 * MH_LANES];
        }
        const float s0 = lane < a.D ? f0 * f0 : 0.f, s1 = lane + MH_LANES < a.D ? f1 * f1 : 0.f;
#pragma unroll
        for (int o = 0; o < 4; ++o) y[o] = mh_group_sum(y[o]);
        const float nrm2 = mh_group_sum(s0 + s1);
        const float extra = __shfl(a.D < MH_LANES ? f0 : a.D < 2 * MH_LANES ? f1 : f2, a.D % MH_LANES, MH_LANES);      // element D: the second confidence's logit
        if (!valid) continue;
#pragma unroll
        for (int o = 0; o < 4; ++o) y[o] += o < a.od ? bias[o] : 0.f;
        if (lane < 3) {
            float r = y[lane];
            if (a.pts_mode != GD_MH_PTS_LINEAR) {
                const float d = sqrtf(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
                r = r / fmaxf(d, 1e-8f) * (a.pts_mode == GD_MH_PTS_SQUARE ? d * d : expm1f(d));
            }
            pts3d[p * 3 + lane] = r;
        }
        const float cv = a.od == 4 ? mh_conf(y[3], a.conf_mode, a.conf_vmin, a.conf_vmax) : 0.f;
        if (lane == 3 && a.od == 4) conf[p] = cv;
        if (lf) {
            const float nrm = a.desc_mode == GD_MH_DESC_NORM ? sqrtf(nrm2) : 1.0f;          // no epsilon, as the reference: a zero vector gives NaN
            if (lane < a.D) desc[p * a.D + lane] = f0 / nrm;
            if (lane + MH_LANES < a.D) desc[p * a.D + lane + MH_LANES] = f1 / nrm;
            if (lane == 4) desc_conf[p] = a.two_confs ? mh_conf(extra, a.dconf_mode, a.dconf_vmin, a.dconf_vmax) : cv;
        }
    }
}

extern "C" int gd_mast3r_head_out(const float* x, const float* w, const float* bias, const float* lf, float* pts3d, float* conf, float* desc,
                                  float* desc_conf, int frames, int H, int W, int Cin, int od, int P, int D, int two_confs, int pts_mode, int conf_mode,
                                  float conf_vmin, float conf_vmax, int desc_mode, int dconf_mode, float dconf_vmin, float dconf_vmax, void* stream) {
    GD_REQUIRE(frames > 0 && H > 0 && W > 0 && Cin > 0, "gd_mast3r_head_out: bad shape frames=%d %dx%d C_in=%d", frames, H, W, Cin);
    GD_REQUIRE(Cin % 8 == 0, "gd_mast3r_head_out: C_in = %d is not a multiple of 8 (the map's rows are moved in 16-byte pieces)", Cin);
    GD_REQUIRE(od == 3 || od == 4, "gd_mast3r_head_out: %d output channels: served are 3 (pts3d) and 4 (pts3d + confidence)", od);
    GD_REQUIRE(pts_mode >= GD_MH_PTS_LINEAR && pts_mode <= GD_MH_PTS_EXP, "gd_mast3r_head_out: unknown pts3d mode code %d", pts_mode);
    GD_REQUIRE(conf_mode >= GD_MH_CONF_EXP && conf_mode <= GD_MH_CONF_RAW, "gd_mast3r_head_out: unknown confidence mode code %d", conf_mode);
    GD_REQUIRE((long)frames * H * (W + 1) < (1L << 31), "gd_mast3r_head_out: pixel rows reach 2^31");
    if (lf) {
        GD_REQUIRE(P >= 1 && P <= 16, "gd_mast3r_head_out: patch size %d: served are 1 .. 16", P);
        GD_REQUIRE(D >= 1 && D <= MH_MAX_D, "gd_mast3r_head_out: %d descriptor channels: served are 1 .. %d", D, MH_MAX_D);
        GD_REQUIRE(two_confs == 0 || two_confs == 1, "gd_mast3r_head_out: two_confs = %d: 0 or 1", two_confs);
        GD_REQUIRE(H % P == 0 && W % P == 0, "gd_mast3r_head_out: the %dx%d map is not a whole number of %d-pixel patches", H, W, P);
        GD_REQUIRE(two_confs || od == 4, "gd_mast3r_head_out: without two_confs desc_conf copies conf, which a 3-channel head does not have");
        GD_REQUIRE(desc_mode == GD_MH_DESC_NORM || desc_mode == GD_MH_DESC_RAW, "gd_mast3r_head_out: unknown descriptor mode code %d", desc_mode);
        GD_REQUIRE(dconf_mode >= GD_MH_CONF_EXP && dconf_mode <= GD_MH_CONF_RAW, "gd_mast3r_head_out: unknown desc_conf mode code %d", dconf_mode);
    }
    GD_REQUIRE(x && w && bias && pts3d && (od == 3 || conf) && ((uintptr_t)x & 15) == 0 && ((uintptr_t)w & 15) == 0,
               "gd_mast3r_head_out: null pointer (x, w, bias, pts3d, conf with 4 channels), or x / w not 16-byte aligned");
    GD_REQUIRE(!lf || (desc && desc_conf && ((uintptr_t)lf & 15) == 0), "gd_mast3r_head_out: desc / desc_conf null, or lf not 16-byte aligned");
    Mast3rHeadArgs a{frames, H, W, Cin, od, lf ? P : 1, lf ? D : 0, lf ? two_confs : 0, pts_mode, conf_mode, desc_mode, dconf_mode,
                     conf_vmin, conf_vmax, dconf_vmin, dconf_vmax};
    hipLaunchKernelGGL(mast3r_head_out_kernel, dim3(dpt_blocks((long)frames * H * W * MH_LANES)), dim3(256), 0, (hipStream_t)stream, x, w, bias, lf, pts3d,
                       conf, desc, desc_conf, a);
    GD_LAUNCH_OK();
    return 0;
}
