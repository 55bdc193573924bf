// Score-CAM (Wang et al., CVPR-W 2020; the gradient-free CAM family of the reference's torchcam_vis.py): every channel of the
// backbone's output, upsampled and min-max scaled, masks the image; the masked images go through the model and every channel
// is weighted by the class probability its mask produced.  Three kernels, each with one fixed order per output element and no
// atomics, so two calls give the same bits.
//
// For one image's features feat NHWC [h][w][C] and channel c,
//   U_c(y, x) = bilinear(feat[:, :, c], H x W, align_corners = False)
// (src = (d + 0.5) in / out - 0.5 clamped at 0, lower index clamped to in - 1, upper index min(lower + 1, in - 1): at_source /
// at_bilerp of attr_common.h, the resize of cam_maps WITHOUT its clamp at 0), lo_c / hi_c = the minimum / maximum of the fp32
// values U_c(y, x) over the H W pixels, span_c = hi_c - lo_c (one fp32 subtraction), and
//   mask_c(y, x) = (U_c(y, x) - lo_c) / span_c        -- ONE subtraction, then ONE correctly rounded division, in this order,
// when span_c > 0 (the channel is LIVE; its mask attains exactly 0 and exactly 1, since U takes the values lo and hi and
// span / span = 1), and 0 everywhere otherwise (DEAD: a constant channel, or one with a NaN / infinity in its range).  U is
// formed by ONE inlined expression (at_source / sc_value) and the mask by one more (sc_mask) wherever they are needed; neither
// is ever stored: C full-resolution masks never exist.  Every index is clamped, so no feature value moves an address.
//
// scorecam_ranges_kernel: ranges[c] = (lo_c, hi_c).  A workgroup takes SC_TC consecutive channels: it reads them for all h w
//   positions coalesced along C into LDS (transposed, odd stride), then each wave owns a channel and walks the H W destination
//   pixels, a butterfly min / max at the end.
// scorecam_mask_images_kernel: out[i][ch][y][x] = image[ch][y][x] mask_{first + i}(y, x).  A workgroup belongs to ONE channel
//   (blockIdx.x) and holds its h w source values and (lo, span) in LDS / registers; the mask value of a pixel is formed once and
//   multiplies all Cin image channels.  W a multiple of 4 and 16-byte aligned pointers: four pixels of a row per thread, 16-byte
//   loads and stores; anything else: one pixel per thread.  A dead channel writes zeros.
// scorecam_accumulate_kernel: acc[k][p] += sum_i live_{first + i} expf(logp[i][cols[k]]) feat[p][first + i].  One thread per
//   position and per tile of SC_KT classes (blockIdx.y), SC_KT accumulators in registers that START from acc and take one fma per
//   live channel in i order (a dead channel is skipped): splitting the channels over several calls at any point gives the bits
//   of one call.  The weights of SC_NP channels at a time are staged in LDS, so n is unbounded.
#include "attr_common.h"

// (SC_MAX_SRC, SC_THREADS, SC_KT, SC_NP, sc_value, sc_scale, sc_live, sc_mask, sc_add_live and sc_check_geometry live in
// attr_common.h: sscam.hip forms the same masks and the same fma chain)
constexpr int SC_TC = 8, SC_RANGE_THREADS = SC_TC * 64;      // channels per workgroup of the range kernel, one wave each

__global__ __launch_bounds__(SC_RANGE_THREADS) void scorecam_ranges_kernel(const float* __restrict__ feat,
                                                                           float* __restrict__ ranges, int h, int w, int C,
                                                                           int H, int W) {
    __shared__ float s_src[SC_TC * (SC_MAX_SRC + 1)];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int hw = h * w, ld = hw | 1;                         // (an odd row stride: the transposing writes spread over banks)
    const int c0 = blockIdx.x * SC_TC;
    for (int i = tid; i < hw * SC_TC; i += SC_RANGE_THREADS) {
        const int p = i / SC_TC, j = i - p * SC_TC;
        if (c0 + j < C) s_src[j * ld + p] = feat[(long)p * C + c0 + j];
    }
    __syncthreads();
    const int c = c0 + wv;
    if (c >= C) return;
    const float* __restrict__ src = s_src + wv * ld;
    const float sy = sc_scale(h, H), sx = sc_scale(w, W);
    float lo = INFINITY, hi = -INFINITY;
    for (int y = 0; y < H; ++y) {
        int y0, y1;
        float ty;
        at_source(y, sy, h, y0, y1, ty);
        const float* r0 = src + y0 * w;
        const float* r1 = src + y1 * w;
        for (int x = lane; x < W; x += 64) {
            int x0, x1;
            float tx;
            at_source(x, sx, w, x0, x1, tx);
            const float v = sc_value(r0, r1, ty, x0, x1, tx);
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    }
    at_wave_minmax(lo, hi);
    if (lane == 0) {
        ranges[2 * (long)c] = lo;
        ranges[2 * (long)c + 1] = hi;
    }
}

extern "C" int scouter_scorecam_ranges_f32(const float* feat, float* ranges, int h, int w, int C, int H, int W, void* stream) {
    SC_REQUIRE(feat && ranges, "scorecam_ranges: null pointer (feat %p, ranges %p)", (const void*)feat, (void*)ranges);
    if (int rc = sc_check_geometry("scorecam_ranges", h, w, C)) return rc;
    SC_REQUIRE(H > 0 && W > 0, "scorecam_ranges: bad arguments (H %d, W %d: each must be at least 1)", H, W);
    SC_REQUIRE((((uintptr_t)feat | (uintptr_t)ranges) & 3) == 0,
               "scorecam_ranges: misaligned pointer (feat and ranges must be 4-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("scorecam_ranges", st, 16.0 * C * (double)H * W, 4.0 * C * ((double)h * w + 2.0));
    hipLaunchKernelGGL(scorecam_ranges_kernel, dim3((unsigned)sc_cdiv(C, SC_TC)), dim3(SC_RANGE_THREADS), 0, st, feat, ranges, h,
                       w, C, H, W);
    return sc_check_launch("scorecam_ranges");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(SC_THREADS) void scorecam_mask_images_kernel(const float* __restrict__ image,
                                                                          const float* __restrict__ feat,
                                                                          const float* __restrict__ ranges,
                                                                          float* __restrict__ out, int first, int Cin, int H,
                                                                          int W, int h, int w, int C) {
    __shared__ float s_src[SC_MAX_SRC];
    const int tid = threadIdx.x;
    const int c = first + blockIdx.x;                          // (the host keeps 0 <= first and first + n <= C)
    for (int p = tid; p < h * w; p += SC_THREADS) s_src[p] = feat[(long)p * C + c];
    const float lo = ranges[2 * (long)c], hi = ranges[2 * (long)c + 1];
    const float span = hi - lo;
    const bool live = sc_live(lo, hi);
    __syncthreads();
    const float sy = sc_scale(h, H), sx = sc_scale(w, W);
    const long plane = (long)H * W;
    float* __restrict__ o = out + (long)blockIdx.x * Cin * plane;
    constexpr int V = VEC ? 4 : 1;
    const int wq = W / V;                                      // (VEC: W is a multiple of 4)
    const long items = (long)H * wq;
    for (long i = (long)blockIdx.y * SC_THREADS + tid; i < items; i += (long)gridDim.y * SC_THREADS) {
        const int y = (int)(i / wq), x = (int)(i - (long)y * wq) * V;
        const long p = (long)y * W + x;
        if (!live) {                                           // (uniform over the workgroup)
            for (int ch = 0; ch < Cin; ++ch) {
                if constexpr (VEC) *(f32x4*)(o + ch * plane + p) = f32x4{0.f, 0.f, 0.f, 0.f};
                else o[ch * plane + p] = 0.f;
            }
            continue;
        }
        int y0, y1;
        float ty;
        at_source(y, sy, h, y0, y1, ty);
        const float* r0 = s_src + y0 * w;
        const float* r1 = s_src + y1 * w;
        float m[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            int x0, x1;
            float tx;
            at_source(x + k, sx, w, x0, x1, tx);
            m[k] = sc_mask(sc_value(r0, r1, ty, x0, x1, tx), lo, span);
        }
        at_scale_channels<VEC>(image, o, plane, p, Cin, m);
    }
}

extern "C" int scouter_scorecam_mask_images_f32(const float* image, const float* feat, const float* ranges, float* out, int first,
                                                int n, int Cin, int H, int W, int h, int w, int C, void* stream) {
    SC_REQUIRE(image && feat && ranges && out, "scorecam_mask_images: null pointer (image %p, feat %p, ranges %p, out %p)",
               (const void*)image, (const void*)feat, (const void*)ranges, (void*)out);
    if (int rc = sc_check_geometry("scorecam_mask_images", h, w, C)) return rc;
    SC_REQUIRE(n > 0 && Cin > 0 && H > 0 && W > 0,
               "scorecam_mask_images: bad arguments (n %d, Cin %d, H %d, W %d: each must be at least 1)", n, Cin, H, W);
    SC_REQUIRE(first >= 0 && (long)first + n <= C, "scorecam_mask_images: channels [%d, %ld) lie outside [0, C = %d)", first,
               (long)first + n, C);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)feat | (uintptr_t)ranges | (uintptr_t)out) & 3) == 0,
               "scorecam_mask_images: misaligned pointer (image, feat, ranges and out must be 4-byte aligned)");
    SC_UNSUPPORTED((long)Cin * H * W < (1L << 31), "scorecam_mask_images: image of %d x %d x %d elements is past the 32-bit offsets",
                   Cin, H, W);
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, SC_THREADS, (uintptr_t)image | (uintptr_t)out);
    const double elems = (double)n * Cin * H * W;
    ScProfScope prof("scorecam_mask_images", st, elems + 18.0 * n * (double)H * W,
                     4.0 * (elems + (double)Cin * H * W + (double)n * (h * w + 2)));
    const dim3 grid((unsigned)n, px.tiles);
    if (px.vec)
        hipLaunchKernelGGL(scorecam_mask_images_kernel<true>, grid, dim3(SC_THREADS), 0, st, image, feat, ranges, out, first, Cin,
                           H, W, h, w, C);
    else
        hipLaunchKernelGGL(scorecam_mask_images_kernel<false>, grid, dim3(SC_THREADS), 0, st, image, feat, ranges, out, first,
                           Cin, H, W, h, w, C);
    return sc_check_launch("scorecam_mask_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS) void scorecam_accumulate_kernel(const float* __restrict__ logp,
                                                                         const int* __restrict__ cols,
                                                                         const float* __restrict__ feat,
                                                                         const float* __restrict__ ranges,
                                                                         float* __restrict__ acc, int first, int n, int n_classes,
                                                                         int K, int hw, int C) {
    __shared__ __attribute__((aligned(16))) float s_w[SC_NP][SC_KT];
    __shared__ int s_live[SC_NP];
    __shared__ int s_col[SC_KT];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.y * SC_KT, kt = min(SC_KT, K - k0);
    at_stage_columns<SC_KT>(cols, k0, kt, n_classes, s_col);
    const int p = blockIdx.x * SC_THREADS + tid;
    const bool mine = p < hw;
    const float* __restrict__ f = feat + (long)(mine ? p : 0) * C + first;
    float a[SC_KT];
    at_load_acc<SC_KT>(acc, hw, p, k0, kt, mine, a);

    for (int n0 = 0; n0 < n; n0 += SC_NP) {
        const int np = min(SC_NP, n - n0);
        __syncthreads();                                        // (s_col is written; the previous piece is consumed)
        at_stage_weights<SC_KT, SC_THREADS>(logp, n0, np, kt, n_classes, s_col, s_w, [](float e) { return e; });
        if (tid < np) {
            const long c = (long)first + n0 + tid;
            s_live[tid] = sc_live(ranges[2 * c], ranges[2 * c + 1]) ? 1 : 0;
        }
        __syncthreads();
        if (mine) sc_add_live(f + n0, s_w, s_live, np, a);
    }
    if (mine) at_store_acc<SC_KT>(acc, hw, p, k0, kt, a);
}

extern "C" int scouter_scorecam_accumulate_f32(const float* logp, const int* cols, const float* feat, const float* ranges,
                                               float* acc, int first, int n, int n_classes, int K, int h, int w, int C,
                                               void* stream) {
    SC_REQUIRE(logp && cols && feat && ranges && acc,
               "scorecam_accumulate: null pointer (logp %p, cols %p, feat %p, ranges %p, acc %p)", (const void*)logp,
               (const void*)cols, (const void*)feat, (const void*)ranges, (void*)acc);
    if (int rc = sc_check_geometry("scorecam_accumulate", h, w, C)) return rc;
    SC_REQUIRE(n > 0 && n_classes > 0 && K > 0,
               "scorecam_accumulate: bad arguments (n %d, n_classes %d, K %d: each must be at least 1)", n, n_classes, K);
    SC_REQUIRE(first >= 0 && (long)first + n <= C, "scorecam_accumulate: channels [%d, %ld) lie outside [0, C = %d)", first,
               (long)first + n, C);
    SC_REQUIRE((((uintptr_t)logp | (uintptr_t)cols | (uintptr_t)feat | (uintptr_t)ranges | (uintptr_t)acc) & 3) == 0,
               "scorecam_accumulate: misaligned pointer (logp, cols, feat, ranges and acc must be 4-byte aligned)");
    const int ktiles = sc_cdiv(K, SC_KT);
    SC_UNSUPPORTED(ktiles <= 65535, "scorecam_accumulate: K = %d classes (at most %d)", K, 65535 * SC_KT);
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)h * w;
    ScProfScope prof("scorecam_accumulate", st, 2.0 * n * px * ktiles * SC_KT,
                     8.0 * K * px + 4.0 * n * ((double)n_classes + px + 2.0));
    hipLaunchKernelGGL(scorecam_accumulate_kernel, dim3((unsigned)sc_cdiv((long)h * w, SC_THREADS), (unsigned)ktiles),
                       dim3(SC_THREADS), 0, st, logp, cols, feat, ranges, acc, first, n, n_classes, K, h * w, C);
    return sc_check_launch("scorecam_accumulate");
}
