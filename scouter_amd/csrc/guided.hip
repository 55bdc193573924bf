// Guided Grad-CAM's product (Selvaraju et al. 2017; captum's GuidedGradCam): an image-space gradient times a class map of the
// backbone's output brought to the image's size,
//   out[b][c][y][x] = grad[b][c][y][x] * up(cam[b])[y][x],
// one fp32 multiplication per element.  grad / out dense NCHW fp32 (out == grad allowed), cam [h][w] dense per image with any
// batch stride (a column t[:, k] of a [B, K, h, w] tensor, as scouter_gradcam_f32 writes it).
//   mode 0 nearest    source index iy = (y h) / H, ix = (x w) / W in integer arithmetic: F.interpolate(mode = "nearest") whenever
//                     H % h == 0 and W % w == 0 (captum's default)
//   mode 1 bilinear   at_source / at_bilerp of attr_common.h on the operands of resize_bilinear_kernel (causal.hip): the same bits
// A thread owns four consecutive x of one row and forms the upsampled value ONCE for the C channels of its pixels: 16-byte
// non-temporal loads of grad (streamed once), 16-byte stores.  W no multiple of 4 or a pointer off a 16-byte boundary: one pixel
// per thread with the same expressions (at_pixel_grid / at_load / at_store).  The map is read through the cache (h w floats per
// image).  Every index is a function of (y, x) alone, so no value moves an address.  No atomics, vector stores only; one fixed
// expression per element, so two calls give the same bits.
#include "attr_common.h"

constexpr int GC_THREADS = 256;
constexpr int GC_NEAREST = 0, GC_BILINEAR = 1;

// grad and out may be the same buffer: neither is __restrict__; an element is read and written by the one thread that owns it
template <bool VEC, int MODE>
__global__ __launch_bounds__(GC_THREADS) void guided_cam_kernel(const float* grad, const float* __restrict__ cam, float* out, int C,
                                                                int H, int W, int h, int w, long cam_stride_b) {
    constexpr int V = VEC ? 4 : 1;
    const long plane = (long)H * W;
    const int wq = W / V;                                                 // (VEC: W is a multiple of 4)
    const long items = (long)H * wq;
    const float* __restrict__ m = cam + (long)blockIdx.x * cam_stride_b;
    const long base = (long)blockIdx.x * C * plane;
    for (long i = (long)blockIdx.y * GC_THREADS + threadIdx.x; i < items; i += (long)gridDim.y * GC_THREADS) {
        const int y = (int)(i / wq), x = (int)(i - (long)y * wq) * V;
        float up[V];
        if constexpr (MODE == GC_BILINEAR) {
            int y0, y1;
            float ty;
            at_source(y, (float)h / (float)H, h, y0, y1, ty);
            const float* r0 = m + (long)y0 * w;
            const float* r1 = m + (long)y1 * w;
#pragma unroll
            for (int q = 0; q < V; ++q) {
                int x0, x1;
                float tx;
                at_source(x + q, (float)w / (float)W, w, x0, x1, tx);
                up[q] = at_bilerp(r0[x0], r0[x1], r1[x0], r1[x1], tx, ty);
            }
        } else {
            const float* r = m + (((long)y * h) / H) * w;                 // (iy <= h - 1 for y <= H - 1)
#pragma unroll
            for (int q = 0; q < V; ++q) up[q] = r[((long)(x + q) * w) / W];
        }
        const long p = (long)y * W + x;
        for (int c = 0; c < C; ++c) {
            float v[V];
            at_load<V, true>(grad + base + c * plane + p, v);
#pragma unroll
            for (int q = 0; q < V; ++q) v[q] *= up[q];
            at_store<V>(out + base + c * plane + p, v);
        }
    }
}

extern "C" int scouter_guided_cam_f32(const float* grad, const float* cam, float* out, int B, int C, int H, int W, int h, int w,
                                      long cam_stride_b, int mode, void* stream) {
    SC_REQUIRE(grad && cam && out, "guided_cam: null pointer (grad %p, cam %p, out %p)", (const void*)grad, (const void*)cam,
               (void*)out);
    SC_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && h > 0 && w > 0, "guided_cam: bad arguments (B %d, C %d, %d x %d, map %d x %d)", B, C,
               H, W, h, w);
    SC_REQUIRE(mode == GC_NEAREST || mode == GC_BILINEAR, "guided_cam: mode %d (0 nearest, 1 bilinear)", mode);
    SC_REQUIRE(B == 1 || cam_stride_b >= (long)h * w, "guided_cam: batch stride %ld of the map is below its %d x %d elements",
               cam_stride_b, h, w);
    SC_REQUIRE((((uintptr_t)grad | (uintptr_t)cam | (uintptr_t)out) & 3) == 0,
               "guided_cam: misaligned pointer (grad, cam and out must be 4-byte aligned)");
    SC_UNSUPPORTED((long)C * H * W < (1L << 31) && (long)h * w < (1L << 31),
                   "guided_cam: image of %d x %d x %d elements or map of %d x %d is past the 32-bit offsets", C, H, W, h, w);
    const long n = (long)B * C * H * W, ncam = (long)(B - 1) * cam_stride_b + (long)h * w;
    SC_REQUIRE(out == grad || out + n <= grad || grad + n <= out, "guided_cam: out overlaps grad without being grad");
    SC_REQUIRE(out + n <= cam || cam + ncam <= out, "guided_cam: out overlaps the map");
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, GC_THREADS, (uintptr_t)grad | (uintptr_t)out);
    ScProfScope prof("guided_cam", st, (double)n, 4.0 * (2.0 * (double)n + (double)B * h * w));
    const dim3 grid((unsigned)B, px.tiles);
#define GC_LAUNCH(VEC, MODE) \
    hipLaunchKernelGGL((guided_cam_kernel<VEC, MODE>), grid, dim3(GC_THREADS), 0, st, grad, cam, out, C, H, W, h, w, cam_stride_b)
    if (px.vec) {
        if (mode == GC_BILINEAR) GC_LAUNCH(true, GC_BILINEAR);
        else GC_LAUNCH(true, GC_NEAREST);
    } else {
        if (mode == GC_BILINEAR) GC_LAUNCH(false, GC_BILINEAR);
        else GC_LAUNCH(false, GC_NEAREST);
    }
#undef GC_LAUNCH
    return sc_check_launch("guided_cam");
}
