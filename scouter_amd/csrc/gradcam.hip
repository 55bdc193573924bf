// Grad-CAM at the backbone's output (reference captum_vis.py: LayerGradCam(model, layer4), relu_attributions=False;
// sloter/utils/grad_cam.py) and the uint8 heat map the reference draws from an attribution (captum_vis.py:51-59,
// show_cam_on_image): two kernels, each with one fixed summation order per output element and no atomics, so two calls give
// the same bits.
//
// gradcam_kernel: ONE workgroup of 1024 threads per image, feat / dfeat NHWC [N = h w][C] fp32.  Both passes are those of
//   gradcampp_kernel (at_column_sums / at_contract_positions of attr_common.h).
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
//   by the same inlined expression (at_source / at_bilerp of attr_common.h, the resize of resize_bilinear and of Score-CAM) --
//   once for the map's minimum and maximum, once for the bytes (AtHeatScale, as heat_maps_kernel) -- and never stored.  After the
//   first min-max scaling the minimum is exactly 0 and the maximum exactly 1 ((hi - lo) / (hi - lo)), so the extrema of
//   max(., min_level) are max(0, min_level) and max(1, min_level): the second scaling needs no second reduction.  A map that
//   is constant at either step is written as zeros.
#include "attr_common.h"

constexpr int CM_THREADS = 256, CM_WAVES = CM_THREADS / 64, CM_MAX_SRC = 32768;

template <bool VEC>
__global__ __launch_bounds__(AT_THREADS) void gradcam_kernel(const float* __restrict__ feat, const float* __restrict__ dfeat,
                                                             float* __restrict__ out, int N, int C, long out_stride, int relu) {
    __shared__ __attribute__((aligned(16))) float s_w[AT_MAX_C];
    __shared__ __attribute__((aligned(16))) float s_part[AT_PART];
    constexpr int V = VEC ? 4 : 1;
    const long img = (long)blockIdx.x * N * C;
    const float* __restrict__ df = dfeat + img;
    const float fN = (float)N;

    // ---- pass 1: channel means
    at_column_sums<V, float, float>(
        [&](int p, int q, const float (&)[V], float (&a)[V]) {
            float g[V];
            at_load<V>(df + (long)p * C + V * q, g);
#pragma unroll
            for (int k = 0; k < V; ++k) a[k] += g[k];
        },
        [&](float a) { return a / fN; }, (const float*)nullptr, s_w, s_part, N, C);

    // ---- pass 2: one wave per position
    at_contract_positions<VEC>(feat + img, s_w, out + (long)blockIdx.x * out_stride, N, C, C / V, relu);
}

extern "C" int scouter_gradcam_f32(const float* feat, const float* dfeat, float* out, int B, int N, int C, long out_stride,
                                   int relu, void* stream) {
    SC_REQUIRE(feat && dfeat && out, "gradcam: null pointer (feat %p, dfeat %p, out %p)", (const void*)feat, (const void*)dfeat,
               (void*)out);
    SC_REQUIRE(B > 0 && N > 0 && C > 0, "gradcam: bad arguments (B %d, N %d, C %d: each must be at least 1)", B, N, C);
    SC_REQUIRE(((uintptr_t)feat & 15) == 0 && ((uintptr_t)dfeat & 15) == 0 && ((uintptr_t)out & 3) == 0,
               "gradcam: misaligned pointer (feat and dfeat 16-byte, out 4-byte aligned)");
    SC_REQUIRE(out_stride >= N || B == 1, "gradcam: output batch stride %ld is below N = %d", out_stride, N);
    SC_UNSUPPORTED(C <= AT_MAX_C, "gradcam: C = %d channels (the channel means live in LDS: at most %d)", C, AT_MAX_C);
    SC_UNSUPPORTED((long)N * C < (1L << 31), "gradcam: image of %d x %d elements is past the 32-bit offsets", N, C);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("gradcam", st, 2.0 * B * (double)N * C * 2.0, 4.0 * B * (2.0 * (double)N * C + N));
    if (C % 4 == 0)
        hipLaunchKernelGGL(gradcam_kernel<true>, dim3((unsigned)B), dim3(AT_THREADS), 0, st, feat, dfeat, out, N, C, out_stride,
                           relu);
    else
        hipLaunchKernelGGL(gradcam_kernel<false>, dim3((unsigned)B), dim3(AT_THREADS), 0, st, feat, dfeat, out, N, C, out_stride,
                           relu);
    return sc_check_launch("gradcam");
}

// ---------------------------------------------------------------------------------------------------------------------------
// max(bilinear, 0) at column (x0, x1, tx) of the two source rows r0 / r1 (LDS) with row weight ty
__device__ __forceinline__ float cm_value(const float* __restrict__ r0, const float* __restrict__ r1, float ty, int x0, int x1,
                                          float tx) {
    return fmaxf(at_bilerp(r0[x0], r0[x1], r1[x0], r1[x1], tx, ty), 0.f);
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
        at_source(y, sy, h, y0, y1, ty);
        const float* r0 = s_src + y0 * w;
        const float* r1 = s_src + y1 * w;
        for (int x = lane; x < W; x += 64) {
            int x0, x1;
            float tx;
            at_source(x, sx, w, x0, x1, tx);
            const float v = cm_value(r0, r1, ty, x0, x1, tx);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    at_block_minmax<CM_WAVES>(lo, hi, s_lo, s_hi);

    // ---- the bytes
    const AtHeatScale scale(lo, hi, min_level);
    unsigned char* __restrict__ dst = out + (long)blockIdx.x * H * W;
    for (int y = wv; y < H; y += CM_WAVES) {
        int y0, y1;
        float ty;
        at_source(y, sy, h, y0, y1, ty);
        const float* r0 = s_src + y0 * w;
        const float* r1 = s_src + y1 * w;
        for (int x = lane; x < W; x += 64) {
            int x0, x1;
            float tx;
            at_source(x, sx, w, x0, x1, tx);
            dst[(long)y * W + x] = scale.byte(cm_value(r0, r1, ty, x0, x1, tx));
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
