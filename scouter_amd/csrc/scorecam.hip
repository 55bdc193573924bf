// The Score-CAM family (the gradient-free CAMs of the reference's torchcam_vis.py): Score-CAM (Wang et al., CVPR-W 2020), SS-CAM
// (Wang et al. 2020, "SS-CAM: Smoothed Score-CAM") and IS-CAM (Naidu et al. 2020, "IS-CAM: Integrated Score-CAM").  Every channel
// of the backbone's output, upsampled and min-max scaled, masks the image; the masked images go through the model N times -- as
// they are (Score-CAM, N = 1), with Gaussian noise added to the mask (SS-CAM) or scaled along a ramp (IS-CAM) -- and every channel
// is weighted by the sum (the mean) of the class probabilities its masks produced.  Four kernels, each with one fixed order per
// output element and no atomics, so two calls give the same bits.
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
// The N C rows of an image form ONE flat stream, row r = sample j = r / C, channel c = r % C; a chunk of at most C consecutive
// rows may straddle a sample boundary, and no two of its rows share a channel.  For row r the masked image is, in fp32 and in
// this order with no contraction,
//   a = scale_j mask_c(y, x)                  scale_j = 1, or with `ramp` (float)((double)(j + 1) (j + 2) / (2 N))
//   nz = sigma z(seed, j, e)                  e = ch H W + y W + x, z the value of noise_images for (seed, sample j, element e)
//   g = a + nz                                (one sum, fused with neither product)
//   out[ch][y][x] = image[ch][y][x] g         (sigma == 0: no noise is formed, out = image a; without the ramp a = mask_c exactly)
// A dead channel writes zeros, noise or not.  The noise depends on the sample and the image element, not on the channel.
//
// scorecam_ranges_kernel: ranges[c] = (lo_c, hi_c).  A workgroup takes SC_TC consecutive channels: it reads them for all h w
//   positions coalesced along C into LDS (transposed, odd stride), then each wave owns a channel and walks the H W destination
//   pixels, a butterfly min / max at the end.
// sscam_mask_images_kernel: a workgroup belongs to ONE row (blockIdx.x) and holds its channel's h w source values and (lo, span)
//   in LDS / registers; the mask value of a pixel is formed once and multiplies all Cin image channels, the noise is formed once
//   per image channel.  W a multiple of 4 and 16-byte aligned pointers: four pixels of a row per thread, 16-byte loads and stores
//   (e is a multiple of 4 there, so the four words of one Philox counter serve them); anything else: one pixel per thread.  Both
//   go through ss_gain, so they give the same bits.
// sscam_weights_kernel: wsum[c][k] += (double)expf(logp[i][cols[k]]), c = (first_row + i) % C, one thread per (i, k): a chunk
//   holds a channel at most once, so no two threads meet, and any split of the stream gives the same bits.
// sscam_contract_kernel: out[k][p] = sum_c live_c (float)(wsum[c][k] norm) feat[p][c].  One thread per position and per tile of
//   SC_KT classes (blockIdx.y), SC_KT accumulators in registers that start at 0 and take one fma per live channel in ascending
//   order (sc_add_live; a dead channel is skipped), the weight rounded from fp64 once.  The weights of SC_NP channels at a time
//   are staged in LDS, so C is unbounded.
#include "attr_common.h"

constexpr int SC_MAX_SRC = 1024;              // source positions h w per channel (they live in LDS)
constexpr int SC_THREADS = 256;
constexpr int SC_KT = 16;                     // classes per thread (accumulators in registers)
constexpr int SC_NP = 32;                     // channels whose weights are staged in LDS at a time
constexpr int SC_TC = 8, SC_RANGE_THREADS = SC_TC * 64;      // channels per workgroup of the range kernel, one wave each

// bilinear value at column (x0, x1, tx) of the two source rows r0 / r1 (LDS) with row weight ty
__device__ __forceinline__ float sc_value(const float* __restrict__ r0, const float* __restrict__ r1, float ty, int x0, int x1,
                                          float tx) {
    return at_bilerp(r0[x0], r0[x1], r1[x0], r1[x1], tx, ty);
}

// in / out of one axis: the scale every kernel hands to at_source
__device__ __forceinline__ float sc_scale(int in, int out) { return (float)in / (float)out; }

__device__ __forceinline__ bool sc_live(float lo, float hi) { return hi - lo > 0.f; }      // (false with a NaN / infinity)

// the mask value of a live channel: (U - lo) / span, span = hi - lo
__device__ __forceinline__ float sc_mask(float u, float lo, float span) { return (u - lo) / span; }

// a[k] = fmaf(s_w[j][k], f[j], a[k]) for the np staged channels in j order, a dead one skipped (s_live: uniform over the
// workgroup); f points at the thread's position, channel of s_w[0]
__device__ __forceinline__ void sc_add_live(const float* __restrict__ f, const float (*s_w)[SC_KT], const int* s_live, int np,
                                            float (&a)[SC_KT]) {
    for (int j = 0; j < np; ++j) {
        if (!s_live[j]) continue;
        at_fma_tile<SC_KT>(s_w[j], f[j], a);
    }
}

// the geometry every call of the family refuses: a channel's h w source values live in LDS, offsets are 32-bit
static inline int sc_check_geometry(const char* what, int h, int w, int C) {
    SC_REQUIRE(h > 0 && w > 0 && C > 0, "%s: bad arguments (h %d, w %d, C %d: each must be at least 1)", what, h, w, C);
    SC_UNSUPPORTED((long)h * w <= SC_MAX_SRC, "%s: source map %d x %d (a channel lives in LDS: at most %d positions)", what, h, w,
                   SC_MAX_SRC);
    SC_UNSUPPORTED((long)h * w * C < (1L << 31), "%s: features of %d x %d x %d elements are past the 32-bit offsets", what, h, w,
                   C);
    return SC_OK;
}

// the scale of sample j of n_samples on IS-CAM's ramp: the partial sum of (t + 1) / N over t <= j, in closed form
__device__ __forceinline__ float ss_ramp(int j, int n_samples) {
    return (float)((double)(j + 1) * (double)(j + 2) / (2.0 * (double)n_samples));
}

// a = scale m: one product
__device__ __forceinline__ float ss_scaled(float scale, float m) {
#pragma clang fp contract(off)
    return scale * m;
}

// g = a + sigma z: one product, then one sum; contraction is switched off here, or the compiler fuses the two
__device__ __forceinline__ float ss_gain(float a, float sigma, float z) {
#pragma clang fp contract(off)
    const float nz = sigma * z;
    return a + nz;
}

// ---------------------------------------------------------------------------------------------------------------------------
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
template <bool VEC, bool NOISE>
__global__ __launch_bounds__(SC_THREADS) void sscam_mask_images_kernel(const float* __restrict__ image,
                                                                       const float* __restrict__ feat,
                                                                       const float* __restrict__ ranges, float* __restrict__ out,
                                                                       int first_row, int n_samples, int ramp, float sigma,
                                                                       unsigned seed_lo, unsigned seed_hi, int Cin, int H, int W,
                                                                       int h, int w, int C) {
    __shared__ float s_src[SC_MAX_SRC];
    const int tid = threadIdx.x;
    const int r = first_row + blockIdx.x;                      // (the host keeps 0 <= first_row and first_row + n <= N C < 2^31)
    const int j = r / C, c = r - j * C;
    for (int p = tid; p < h * w; p += SC_THREADS) s_src[p] = feat[(long)p * C + c];
    const float lo = ranges[2 * (long)c], hi = ranges[2 * (long)c + 1];
    const float span = hi - lo;
    const bool live = sc_live(lo, hi);
    const float scale = ramp ? ss_ramp(j, n_samples) : 1.f;
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
        float a[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            int x0, x1;
            float tx;
            at_source(x + k, sx, w, x0, x1, tx);
            a[k] = ss_scaled(scale, sc_mask(sc_value(r0, r1, ty, x0, x1, tx), lo, span));
        }
        if constexpr (!NOISE) {
            at_scale_channels<VEC>(image, o, plane, p, Cin, a);
        } else {
            for (int ch = 0; ch < Cin; ++ch) {
                const long e = ch * plane + p;                 // (VEC: a multiple of 4, as plane and p are)
                float z[V], g[V];
                ib_noise<V>(e, (unsigned)j, seed_lo, seed_hi, z);
#pragma unroll
                for (int k = 0; k < V; ++k) g[k] = ss_gain(a[k], sigma, z[k]);
                at_scale_channels<VEC>(image + ch * plane, o + ch * plane, plane, p, 1, g);
            }
        }
    }
}

extern "C" int scouter_sscam_mask_images_f32(const float* image, const float* feat, const float* ranges, float* out,
                                             int first_row, int n, int n_samples, int ramp, float sigma, int seed_lo, int seed_hi,
                                             int Cin, int H, int W, int h, int w, int C, void* stream) {
    SC_REQUIRE(image && feat && ranges && out, "sscam_mask_images: null pointer (image %p, feat %p, ranges %p, out %p)",
               (const void*)image, (const void*)feat, (const void*)ranges, (void*)out);
    if (int rc = sc_check_geometry("sscam_mask_images", h, w, C)) return rc;
    SC_REQUIRE(n > 0 && n_samples > 0 && Cin > 0 && H > 0 && W > 0,
               "sscam_mask_images: bad arguments (n %d, n_samples %d, Cin %d, H %d, W %d: each must be at least 1)", n, n_samples,
               Cin, H, W);
    SC_REQUIRE(n <= C, "sscam_mask_images: a chunk of n = %d rows holds a channel twice (at most C = %d)", n, C);
    SC_UNSUPPORTED((long)n_samples * C < (1L << 31), "sscam_mask_images: a stream of %d x %d rows is past the 32-bit row index",
                   n_samples, C);
    SC_REQUIRE(first_row >= 0 && (long)first_row + n <= (long)n_samples * C,
               "sscam_mask_images: rows [%d, %ld) lie outside [0, n_samples C = %ld)", first_row, (long)first_row + n,
               (long)n_samples * C);
    SC_REQUIRE(sigma >= 0.f && sigma < INFINITY, "sscam_mask_images: sigma %g must be finite and not negative", (double)sigma);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)feat | (uintptr_t)ranges | (uintptr_t)out) & 3) == 0,
               "sscam_mask_images: misaligned pointer (image, feat, ranges and out must be 4-byte aligned)");
    SC_UNSUPPORTED((long)Cin * H * W < (1L << 31), "sscam_mask_images: image of %d x %d x %d elements is past the 32-bit offsets",
                   Cin, H, W);
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, SC_THREADS, (uintptr_t)image | (uintptr_t)out);
    const double elems = (double)n * Cin * H * W;
    const bool noise = sigma > 0.f;
    ScProfScope prof(noise ? "sscam_mask_images<noise>" : "sscam_mask_images", st,
                     (noise ? 100.0 : 1.0) * elems + 19.0 * n * (double)H * W,
                     4.0 * (elems + (double)Cin * H * W + (double)n * (h * w + 2)));
    const dim3 grid((unsigned)n, px.tiles);
    const unsigned klo = (unsigned)seed_lo, khi = (unsigned)seed_hi;
#define SS_LAUNCH(VEC, NOISE)                                                                                                   \
    hipLaunchKernelGGL((sscam_mask_images_kernel<VEC, NOISE>), grid, dim3(SC_THREADS), 0, st, image, feat, ranges, out, first_row, \
                       n_samples, ramp, sigma, klo, khi, Cin, H, W, h, w, C)
    if (px.vec) {
        if (noise) SS_LAUNCH(true, true);
        else SS_LAUNCH(true, false);
    } else {
        if (noise) SS_LAUNCH(false, true);
        else SS_LAUNCH(false, false);
    }
#undef SS_LAUNCH
    return sc_check_launch("sscam_mask_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS) void sscam_weights_kernel(const float* __restrict__ logp, const int* __restrict__ cols,
                                                                   double* __restrict__ wsum, int first_row, int n, int n_classes,
                                                                   int K, int C) {
    const int t = blockIdx.x * SC_THREADS + threadIdx.x;       // (the host keeps n K < 2^31)
    if (t >= n * K) return;
    const int i = t / K, k = t - i * K;
    const int col = min(max(cols[k], 0), n_classes - 1);       // (the caller refuses an index outside [0, n_classes))
    const int c = (int)(((long)first_row + i) % C);
    wsum[(long)c * K + k] += (double)expf(logp[(long)i * n_classes + col]);
}

extern "C" int scouter_sscam_weights_f64(const float* logp, const int* cols, double* wsum, int first_row, int n, int n_classes,
                                         int K, int C, void* stream) {
    SC_REQUIRE(logp && cols && wsum, "sscam_weights: null pointer (logp %p, cols %p, wsum %p)", (const void*)logp,
               (const void*)cols, (void*)wsum);
    SC_REQUIRE(n > 0 && n_classes > 0 && K > 0 && C > 0,
               "sscam_weights: bad arguments (n %d, n_classes %d, K %d, C %d: each must be at least 1)", n, n_classes, K, C);
    SC_REQUIRE(n <= C, "sscam_weights: a chunk of n = %d rows holds a channel twice (at most C = %d)", n, C);
    SC_REQUIRE(first_row >= 0, "sscam_weights: first_row %d is negative", first_row);
    SC_REQUIRE((((uintptr_t)logp | (uintptr_t)cols) & 3) == 0 && ((uintptr_t)wsum & 7) == 0,
               "sscam_weights: misaligned pointer (logp and cols must be 4-byte aligned, wsum 8-byte)");
    SC_UNSUPPORTED((long)n * K < (1L << 31) && (long)n * n_classes < (1L << 31) && (long)C * K < (1L << 31),
                   "sscam_weights: n %d x K %d, n x n_classes %d or C %d x K elements are past the 32-bit offsets", n, K,
                   n_classes, C);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("sscam_weights", st, 2.0 * n * K, 20.0 * n * K + 4.0 * K);
    hipLaunchKernelGGL(sscam_weights_kernel, dim3((unsigned)sc_cdiv((long)n * K, SC_THREADS)), dim3(SC_THREADS), 0, st, logp, cols,
                       wsum, first_row, n, n_classes, K, C);
    return sc_check_launch("sscam_weights");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS) void sscam_contract_kernel(const double* __restrict__ wsum, const float* __restrict__ feat,
                                                                    const float* __restrict__ ranges, float* __restrict__ out,
                                                                    double norm, int K, int hw, int C) {
    __shared__ __attribute__((aligned(16))) float s_w[SC_NP][SC_KT];
    __shared__ int s_live[SC_NP];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.y * SC_KT, kt = min(SC_KT, K - k0);
    const int p = blockIdx.x * SC_THREADS + tid;
    const bool mine = p < hw;
    const float* __restrict__ f = feat + (long)(mine ? p : 0) * C;
    float a[SC_KT];
#pragma unroll
    for (int k = 0; k < SC_KT; ++k) a[k] = 0.f;

    for (int c0 = 0; c0 < C; c0 += SC_NP) {
        const int np = min(SC_NP, C - c0);
        __syncthreads();                                        // (the previous piece is consumed)
        for (int i = tid; i < np * SC_KT; i += SC_THREADS) {
            const int j = i / SC_KT, k = i - j * SC_KT;
            s_w[j][k] = k < kt ? (float)(wsum[(long)(c0 + j) * K + k0 + k] * norm) : 0.f;
        }
        if (tid < np) {
            const long c = (long)c0 + tid;
            s_live[tid] = sc_live(ranges[2 * c], ranges[2 * c + 1]) ? 1 : 0;
        }
        __syncthreads();
        if (mine) sc_add_live(f + c0, s_w, s_live, np, a);
    }
    if (mine) at_store_acc<SC_KT>(out, hw, p, k0, kt, a);
}

extern "C" int scouter_sscam_contract_f32(const double* wsum, const float* feat, const float* ranges, float* out, double norm,
                                          int K, int h, int w, int C, void* stream) {
    SC_REQUIRE(wsum && feat && ranges && out, "sscam_contract: null pointer (wsum %p, feat %p, ranges %p, out %p)",
               (const void*)wsum, (const void*)feat, (const void*)ranges, (void*)out);
    if (int rc = sc_check_geometry("sscam_contract", h, w, C)) return rc;
    SC_REQUIRE(K > 0, "sscam_contract: bad arguments (K %d must be at least 1)", K);
    SC_REQUIRE(norm == norm && norm - norm == 0.0, "sscam_contract: norm %g must be finite", norm);
    SC_REQUIRE((((uintptr_t)feat | (uintptr_t)ranges | (uintptr_t)out) & 3) == 0 && ((uintptr_t)wsum & 7) == 0,
               "sscam_contract: misaligned pointer (feat, ranges and out must be 4-byte aligned, wsum 8-byte)");
    const int ktiles = sc_cdiv(K, SC_KT);
    SC_UNSUPPORTED(ktiles <= 65535, "sscam_contract: K = %d classes (at most %d)", K, 65535 * SC_KT);
    SC_UNSUPPORTED((long)C * K < (1L << 31), "sscam_contract: weights of %d x %d elements are past the 32-bit offsets", C, K);
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)h * w;
    ScProfScope prof("sscam_contract", st, 2.0 * C * px * ktiles * SC_KT, 4.0 * K * px + 8.0 * C * K + 4.0 * C * (px + 2.0));
    hipLaunchKernelGGL(sscam_contract_kernel, dim3((unsigned)sc_cdiv((long)h * w, SC_THREADS), (unsigned)ktiles), dim3(SC_THREADS),
                       0, st, wsum, feat, ranges, out, norm, K, h * w, C);
    return sc_check_launch("sscam_contract");
}
