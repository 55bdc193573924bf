// Grad-CAM at the backbone's output (reference captum_vis.py: LayerGradCam(model, layer4), relu_attributions=False;
// sloter/utils/grad_cam.py) and the uint8 heat map the reference draws from an attribution (captum_vis.py:51-59,
// show_cam_on_image): two kernels, each with one fixed summation order per output element and no atomics, so two calls give
// the same bits.
//
// gradcam_kernel: ONE workgroup of 1024 threads per image, feat / dfeat NHWC [N = h w][C] fp32.
//   pass 1: wbar[c] = (sum_p dfeat[p][c]) / N.  The columns (float4 columns when C is a multiple of 4, single channels
//           otherwise) are spread over the threads, a wave reads 64 consecutive columns of one position (1 KiB); when there
//           are fewer columns than threads the positions are dealt to G = threads / columns groups, whose partial sums meet in
//           LDS and are added in group order.  wbar stays in LDS (C <= 8192: 32 KiB); dfeat is read once.
//   pass 2: out[p] = sum_c wbar[c] feat[p][c], one wave per position: a lane takes every 64th column, the 64 partial sums
//           meet in a butterfly.  feat is read once; out is written through a batch stride (a column of a [B][K][N] tensor).
//   Rounding: N - 1 additions and one division per mean, then one fma per channel and 6 butterfly additions: below the
//   worst-case fp32 bound (N + C + 4) 2^-24 sum_c |wbar_c| |feat_c| of any summation order.
//
// cam_maps_kernel: ONE workgroup of 256 threads per map, the h x w source in LDS (<= 32768 elements).  The upsampled value
//   v(y, x) = max(bilinear(y, x), 0) (align_corners = False: src = (dst + 0.5) in / out - 0.5, clamped at 0) is formed twice
//   by the same inlined expression -- once for the map's minimum and maximum, once for the bytes -- and never stored.  After the
//   first min-max scaling the minimum is exactly 0 and the maximum exactly 1 ((hi - lo) / (hi - lo)), so the extrema of
//   max(., min_level) are max(0, min_level) and max(1, min_level): the second scaling needs no second reduction.  A map that
//   is constant at either step is written as zeros.
#include "common.h"

constexpr int GC_THREADS = 1024, GC_WAVES = GC_THREADS / 64, GC_MAX_C = 8192;
constexpr int CM_THREADS = 256, CM_WAVES = CM_THREADS / 64, CM_MAX_SRC = 32768;

template <bool VEC>
__global__ __launch_bounds__(GC_THREADS) void gradcam_kernel(const float* __restrict__ feat, const float* __restrict__ dfeat,
                                                             float* __restrict__ out, int N, int C, long out_stride, int relu) {
    __shared__ __attribute__((aligned(16))) float s_w[GC_MAX_C];
    __shared__ __attribute__((aligned(16))) float s_part[GC_THREADS * 4];
    constexpr int V = VEC ? 4 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long img = (long)blockIdx.x * N * C;
    const float* __restrict__ df = dfeat + img;
    const float* __restrict__ ft = feat + img;
    const int cols = C / V;                                   // (VEC: C is a multiple of 4)
    const float fN = (float)N;

    // ---- pass 1: channel means
    if (cols >= GC_THREADS) {
        for (int q = tid; q < cols; q += GC_THREADS) {
            float a[V];
#pragma unroll
            for (int k = 0; k < V; ++k) a[k] = 0.f;
#pragma unroll 4
            for (int p = 0; p < N; ++p) {
                if constexpr (VEC) {
                    const f32x4 v = *(const f32x4*)(df + (long)p * C + 4 * q);
#pragma unroll
                    for (int k = 0; k < 4; ++k) a[k] += v[k];
                } else {
                    a[0] += df[(long)p * C + q];
                }
            }
#pragma unroll
            for (int k = 0; k < V; ++k) s_w[V * q + k] = a[k] / fN;
        }
    } else {
        int G = GC_THREADS / cols;
        if (G > N) G = N;
        const int g = tid / cols, q = tid - g * cols;
        if (g < G) {
            float a[V];
#pragma unroll
            for (int k = 0; k < V; ++k) a[k] = 0.f;
#pragma unroll 4
            for (int p = g; p < N; p += G) {
                if constexpr (VEC) {
                    const f32x4 v = *(const f32x4*)(df + (long)p * C + 4 * q);
#pragma unroll
                    for (int k = 0; k < 4; ++k) a[k] += v[k];
                } else {
                    a[0] += df[(long)p * C + q];
                }
            }
#pragma unroll
            for (int k = 0; k < V; ++k) s_part[g * C + V * q + k] = a[k];        // (G * C <= GC_THREADS * V)
        }
        __syncthreads();
        for (int c = tid; c < C; c += GC_THREADS) {
            float a = s_part[c];
            for (int j = 1; j < G; ++j) a += s_part[j * C + c];
            s_w[c] = a / fN;
        }
    }
    __syncthreads();

    // ---- pass 2: one wave per position
    float* __restrict__ o = out + (long)blockIdx.x * out_stride;
    for (int p = wv; p < N; p += GC_WAVES) {
        const float* __restrict__ row = ft + (long)p * C;
        float a = 0.f;
        for (int q = lane; q < cols; q += 64) {
            if constexpr (VEC) {
                const f32x4 v = *(const f32x4*)(row + 4 * q);
                const f32x4 w = *(const f32x4*)(s_w + 4 * q);
#pragma unroll
                for (int k = 0; k < 4; ++k) a = fmaf(v[k], w[k], a);
            } else {
                a = fmaf(row[q], s_w[q], a);
            }
        }
        a = wave_sum(a);
        if (lane == 0) o[p] = relu ? fmaxf(a, 0.f) : a;
    }
}

extern "C" int scouter_gradcam_f32(const float* feat, const float* dfeat, float* out, int B, int N, int C, long out_stride,
                                   int relu, void* stream) {
    SC_REQUIRE(feat && dfeat && out, "gradcam: null pointer (feat %p, dfeat %p, out %p)", (const void*)feat, (const void*)dfeat,
               (void*)out);
    SC_REQUIRE(B > 0 && N > 0 && C > 0, "gradcam: bad arguments (B %d, N %d, C %d: each must be at least 1)", B, N, C);
    SC_REQUIRE(((uintptr_t)feat & 15) == 0 && ((uintptr_t)dfeat & 15) == 0 && ((uintptr_t)out & 3) == 0,
               "gradcam: misaligned pointer (feat and dfeat 16-byte, out 4-byte aligned)");
    SC_REQUIRE(out_stride >= N || B == 1, "gradcam: output batch stride %ld is below N = %d", out_stride, N);
    SC_UNSUPPORTED(C <= GC_MAX_C, "gradcam: C = %d channels (the channel means live in LDS: at most %d)", C, GC_MAX_C);
    SC_UNSUPPORTED((long)N * C < (1L << 31), "gradcam: image of %d x %d elements is past the 32-bit offsets", N, C);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("gradcam", st, 2.0 * B * (double)N * C * 2.0, 4.0 * B * (2.0 * (double)N * C + N));
    if (C % 4 == 0)
        hipLaunchKernelGGL(gradcam_kernel<true>, dim3((unsigned)B), dim3(GC_THREADS), 0, st, feat, dfeat, out, N, C, out_stride,
                           relu);
    else
        hipLaunchKernelGGL(gradcam_kernel<false>, dim3((unsigned)B), dim3(GC_THREADS), 0, st, feat, dfeat, out, N, C, out_stride,
                           relu);
    return sc_check_launch("gradcam");
}

// ---------------------------------------------------------------------------------------------------------------------------
// source coordinate of destination index d (align_corners = False): the lower neighbour, the upper one and its weight
__device__ __forceinline__ void cm_source(int d, float scale, int n, int& i0, int& i1, float& t) {
    float s = fmaf((float)d + 0.5f, scale, -0.5f);
    s = fmaxf(s, 0.f);
    i0 = min((int)s, n - 1);
    i1 = min(i0 + 1, n - 1);
    t = s - (float)i0;
}

// max(bilinear, 0) at column (x0, x1, tx) of the two source rows r0 / r1 (LDS) with row weight ty
__device__ __forceinline__ float cm_value(const float* __restrict__ r0, const float* __restrict__ r1, float ty, int x0, int x1,
                                          float tx) {
    const float a0 = r0[x0], a1 = r0[x1], b0 = r1[x0], b1 = r1[x1];
    const float top = fmaf(tx, a1 - a0, a0), bot = fmaf(tx, b1 - b0, b0);
    return fmaxf(fmaf(ty, bot - top, top), 0.f);
}

__global__ __launch_bounds__(CM_THREADS) void cam_maps_kernel(const float* __restrict__ cam, unsigned char* __restrict__ out,
                                                              int h, int w, int H, int W, float min_level) {
    extern __shared__ __attribute__((aligned(16))) float s_src[];         // [h * w]
    __shared__ float s_lo[CM_WAVES], s_hi[CM_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* __restrict__ src = cam + (long)blockIdx.x * h * w;
    for (int i = tid; i < h * w; i += CM_THREADS) s_src[i] = src[i];
    __syncthreads();
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;

    // ---- the extrema of v
    float lo = INFINITY, hi = -INFINITY;
    for (int y = wv; y < H; y += CM_WAVES) {
        int y0, y1;
        float ty;
        cm_source(y, sy, h, y0, y1, ty);
        const float* r0 = s_src + y0 * w;
        const float* r1 = s_src + y1 * w;
        for (int x = lane; x < W; x += 64) {
            int x0, x1;
            float tx;
            cm_source(x, sx, w, x0, x1, tx);
            const float v = cm_value(r0, r1, ty, x0, x1, tx);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if (lane == 0) { s_lo[wv] = lo; s_hi[wv] = hi; }
    __syncthreads();
    lo = s_lo[0]; hi = s_hi[0];
#pragma unroll
    for (int k = 1; k < CM_WAVES; ++k) { lo = fminf(lo, s_lo[k]); hi = fmaxf(hi, s_hi[k]); }

    // ---- the two scalings as one affine map of v: ((v - lo) / span1 raised to lo2, minus lo2) / span2
    const float span1 = hi - lo;
    const float lo2 = fmaxf(0.f, min_level), span2 = fmaxf(1.f, min_level) - lo2;
    const bool flat = !(span1 > 0.f) || !(span2 > 0.f);                   // (also a map with a NaN / infinity in it)
    unsigned char* __restrict__ dst = out + (long)blockIdx.x * H * W;
    for (int y = wv; y < H; y += CM_WAVES) {
        int y0, y1;
        float ty;
        cm_source(y, sy, h, y0, y1, ty);
        const float* r0 = s_src + y0 * w;
        const float* r1 = s_src + y1 * w;
        for (int x = lane; x < W; x += 64) {
            int x0, x1;
            float tx;
            cm_source(x, sx, w, x0, x1, tx);
            float c = 0.f;
            if (!flat) {
                const float v = cm_value(r0, r1, ty, x0, x1, tx);
                const float a = fmaxf((v - lo) / span1, min_level);
                c = fminf(fmaxf((a - lo2) / span2, 0.f), 1.f);
            }
            dst[(long)y * W + x] = (unsigned char)(int)(255.f * c);
        }
    }
}

extern "C" int scouter_cam_maps_u8(const float* cam, unsigned char* out, int M, int h, int w, int H, int W, float min_level,
                                   void* stream) {
    SC_REQUIRE(cam && out, "cam_maps: null pointer (cam %p, out %p)", (const void*)cam, (void*)out);
    SC_REQUIRE(((uintptr_t)cam & 3) == 0, "cam_maps: misaligned pointer (cam must be 4-byte aligned)");
    SC_REQUIRE(M > 0 && h > 0 && w > 0 && H > 0 && W > 0, "cam_maps: bad arguments (M %d, %d x %d -> %d x %d)", M, h, w, H, W);
    SC_REQUIRE(min_level == min_level, "cam_maps: min_level is not a number");
    SC_UNSUPPORTED((long)h * w <= CM_MAX_SRC, "cam_maps: source map %d x %d (it lives in LDS: at most %d elements)", h, w,
                   CM_MAX_SRC);
    SC_UNSUPPORTED((long)H * W < (1L << 31), "cam_maps: output map %d x %d is past the 32-bit offsets", H, W);
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)h * w * sizeof(float);
    sc_dyn_lds((const void*)cam_maps_kernel, lds);
    ScProfScope prof("cam_maps", st, 2.0 * 12.0 * M * (double)H * W, (double)M * (4.0 * h * w + (double)H * W));
    hipLaunchKernelGGL(cam_maps_kernel, dim3((unsigned)M), dim3(CM_THREADS), lds, st, cam, out, h, w, H, W, min_level);
    return sc_check_launch("cam_maps");
}
