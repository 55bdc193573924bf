// RISE (Petsiuk et al. 2018; reference torchcam_vis.py: torchray.attribution.rise): saliency from N smooth random masks, and the
// heat map of a full-resolution attribution.  Three kernels, each with one fixed summation order per output element and no
// atomics, so two calls give the same bits.
//
// Mask n is an s x s grid of bytes in {0, 1} and a shift (dy, dx).  With cell = ceil(size / s) and U = (s + 1) cell per axis,
//   mask_n(y, x) = bilinear(grid_n, U_h x U_w, align_corners = False)[y + dy, x + dx],  0 <= dy < cell_h, 0 <= dx < cell_w
// (src = (d + 0.5) s / U - 0.5 clamped at 0, lower index clamped to s - 1, upper index min(lower + 1, s - 1): at_source of
// attr_common.h).  The value is formed by ONE inlined expression (at_source / rs_mask) wherever it is needed and never stored:
// N full-resolution masks never exist.  Every index is clamped, so a shift outside its range reads no byte outside the grid.
//
// rise_mask_images_kernel: out[n][c][y][x] = image[c][y][x] mask_n(y, x).  A workgroup belongs to ONE mask (blockIdx.x) and
//   holds its s^2 bytes in LDS; the mask value of a pixel is formed once and multiplies all C channels.  W a multiple of 4 and
//   16-byte aligned pointers: four pixels of a row per thread, 16-byte loads and stores; anything else: one pixel per thread.
// rise_accumulate_kernel: acc[k][y][x] += sum_n (scale expf(logp[n][cols[k]])) mask_n(y, x).  One thread per pixel and per
//   tile of RS_KT classes (blockIdx.y), RS_KT accumulators in registers that START from acc and take one fma per mask in n
//   order: splitting the masks over several calls at any point gives the bits of one call.  The weights and grid bytes of
//   RS_NP masks at a time are staged in LDS, so N is unbounded.
// heat_maps_kernel: the drawing steps of cam_maps_kernel (gradcam.hip) without the resize and without an LDS source: ONE
//   workgroup per map reads it twice from memory (extrema of max(v, 0), then the bytes).  Both kernels reduce with
//   at_block_minmax and scale with AtHeatScale of attr_common.h: a map cam_maps takes at its own size gets the same bytes.
#include "attr_common.h"

constexpr int RS_MAX_S = 16;
constexpr int RS_THREADS = 256;
constexpr int RS_KT = 16;                     // classes per thread (accumulators in registers)
constexpr int RS_NP = 32;                     // masks staged in LDS at a time
constexpr int HM_THREADS = 1024, HM_WAVES = HM_THREADS / 64;

// bilinear value of the byte grid g [s][s] (LDS) between rows y0 / y1 (weight ty) and columns x0 / x1 (weight tx)
__device__ __forceinline__ float rs_mask(const unsigned char* __restrict__ g, int s, int y0, int y1, float ty, int x0, int x1,
                                         float tx) {
    return at_bilerp((float)g[y0 * s + x0], (float)g[y0 * s + x1], (float)g[y1 * s + x0], (float)g[y1 * s + x1], tx, ty);
}

// s / U of one axis: the scale every kernel hands to at_source
__host__ __device__ __forceinline__ float rs_scale(int size, int s) {
    const int cell = (size + s - 1) / s;
    return (float)s / (float)((s + 1) * cell);
}

template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void rise_mask_images_kernel(const float* __restrict__ image,
                                                                      const unsigned char* __restrict__ grids,
                                                                      const int* __restrict__ shifts, float* __restrict__ out,
                                                                      int C, int H, int W, int s) {
    __shared__ unsigned char s_g[RS_MAX_S * RS_MAX_S];
    const int n = blockIdx.x, tid = threadIdx.x;
    if (tid < s * s) s_g[tid] = grids[(long)n * s * s + tid];
    const int dy = shifts[2 * (long)n], dx = shifts[2 * (long)n + 1];
    __syncthreads();
    const float sy = rs_scale(H, s), sx = rs_scale(W, s);
    const long plane = (long)H * W;
    float* __restrict__ o = out + (long)n * C * plane;
    constexpr int V = VEC ? 4 : 1;
    const int wq = W / V;                                      // (VEC: W is a multiple of 4)
    const long items = (long)H * wq;
    for (long i = (long)blockIdx.y * RS_THREADS + tid; i < items; i += (long)gridDim.y * RS_THREADS) {
        const int y = (int)(i / wq), x = (int)(i - (long)y * wq) * V;
        int y0, y1;
        float ty;
        at_source(y + dy, sy, s, y0, y1, ty);
        float m[V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            int x0, x1;
            float tx;
            at_source(x + k + dx, sx, s, x0, x1, tx);
            m[k] = rs_mask(s_g, s, y0, y1, ty, x0, x1, tx);
        }
        at_scale_channels<VEC>(image, o, plane, (long)y * W + x, C, m);
    }
}

static int rs_check_grid(const char* what, int H, int W, int s) {
    SC_REQUIRE(H > 0 && W > 0, "%s: bad arguments (H %d, W %d: each must be at least 1)", what, H, W);
    SC_REQUIRE(s >= 1 && s <= RS_MAX_S, "%s: grid size s = %d (1 <= s <= %d)", what, s, RS_MAX_S);
    SC_REQUIRE(s <= H && s <= W, "%s: grid size s = %d is above min(H, W) = min(%d, %d)", what, s, H, W);
    return SC_OK;
}

extern "C" int scouter_rise_mask_images_f32(const float* image, const unsigned char* grids, const int* shifts, float* out, int N,
                                            int C, int H, int W, int s, void* stream) {
    SC_REQUIRE(image && grids && shifts && out, "rise_mask_images: null pointer (image %p, grids %p, shifts %p, out %p)",
               (const void*)image, (const void*)grids, (const void*)shifts, (void*)out);
    SC_REQUIRE(N > 0 && C > 0, "rise_mask_images: bad arguments (N %d, C %d: each must be at least 1)", N, C);
    if (int rc = rs_check_grid("rise_mask_images", H, W, s)) return rc;
    SC_REQUIRE(((uintptr_t)image & 3) == 0 && ((uintptr_t)out & 3) == 0 && ((uintptr_t)shifts & 3) == 0,
               "rise_mask_images: misaligned pointer (image, out and shifts must be 4-byte aligned)");
    SC_UNSUPPORTED((long)C * H * W < (1L << 31), "rise_mask_images: image of %d x %d x %d elements is past the 32-bit offsets", C,
                   H, W);
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, RS_THREADS, (uintptr_t)image | (uintptr_t)out);
    const double elems = (double)N * C * H * W;
    ScProfScope prof("rise_mask_images", st, elems + 14.0 * N * (double)H * W, 4.0 * (elems + (double)C * H * W));
    const dim3 grid((unsigned)N, px.tiles);
    if (px.vec)
        hipLaunchKernelGGL(rise_mask_images_kernel<true>, grid, dim3(RS_THREADS), 0, st, image, grids, shifts, out, C, H, W, s);
    else
        hipLaunchKernelGGL(rise_mask_images_kernel<false>, grid, dim3(RS_THREADS), 0, st, image, grids, shifts, out, C, H, W, s);
    return sc_check_launch("rise_mask_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
// The staging of rise_accumulate_kernel: the class columns clamped, the weights of a piece of masks in LDS, KT class
// accumulators in registers per thread that START from acc (at_store_acc of attr_common.h writes them back).

// s_col[k] = the clamped column of class k0 + k, k < kt (the host refuses an index outside [0, n_classes))
template <int KT>
__device__ __forceinline__ void rs_stage_columns(const int* __restrict__ cols, int k0, int kt, int n_classes, int* s_col) {
    const int tid = threadIdx.x;
    if (tid < KT) {
        int c = tid < kt ? cols[k0 + tid] : 0;
        s_col[tid] = min(max(c, 0), n_classes - 1);
    }
}

// s_w[j][k] = factor(expf(logp[n0 + j][s_col[k]])) for the np terms of a piece, 0 for k >= kt
template <int KT, int THREADS, typename Factor>
__device__ __forceinline__ void rs_stage_weights(const float* __restrict__ logp, int n0, int np, int kt, int n_classes,
                                                 const int* s_col, float (*s_w)[KT], Factor factor) {
    for (int i = threadIdx.x; i < np * KT; i += THREADS) {
        const int j = i / KT, k = i - j * KT;
        s_w[j][k] = k < kt ? factor(expf(logp[(long)(n0 + j) * n_classes + s_col[k]])) : 0.f;
    }
}

// a[k] = acc[k0 + k][p] for the kt classes of a thread that owns element p of the plane (mine), else 0
template <int KT>
__device__ __forceinline__ void rs_load_acc(const float* __restrict__ acc, long plane, long p, int k0, int kt, bool mine,
                                            float (&a)[KT]) {
#pragma unroll
    for (int k = 0; k < KT; ++k) a[k] = (mine && k < kt) ? acc[(long)(k0 + k) * plane + p] : 0.f;
}

__global__ __launch_bounds__(RS_THREADS) void rise_accumulate_kernel(const float* __restrict__ logp, const int* __restrict__ cols,
                                                                     const unsigned char* __restrict__ grids,
                                                                     const int* __restrict__ shifts, float* __restrict__ acc,
                                                                     int N, int n_classes, int K, int H, int W, int s,
                                                                     float scale) {
    __shared__ __attribute__((aligned(16))) float s_w[RS_NP][RS_KT];
    __shared__ unsigned char s_g[RS_NP][RS_MAX_S * RS_MAX_S];
    __shared__ int s_shift[RS_NP][2];
    __shared__ int s_col[RS_KT];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.y * RS_KT, kt = min(RS_KT, K - k0), ss = s * s;
    rs_stage_columns<RS_KT>(cols, k0, kt, n_classes, s_col);
    const long plane = (long)H * W;
    const long p = (long)blockIdx.x * RS_THREADS + tid;
    const bool live = p < plane;
    const int y = live ? (int)(p / W) : 0, x = live ? (int)(p - (long)y * W) : 0;
    const float sy = rs_scale(H, s), sx = rs_scale(W, s);
    float a[RS_KT];
    rs_load_acc<RS_KT>(acc, plane, p, k0, kt, live, a);

    for (int n0 = 0; n0 < N; n0 += RS_NP) {
        const int np = min(RS_NP, N - n0);
        __syncthreads();                                        // (s_col is written; the previous piece is consumed)
        rs_stage_weights<RS_KT, RS_THREADS>(logp, n0, np, kt, n_classes, s_col, s_w, [scale](float e) { return scale * e; });
        for (int i = tid; i < np * ss; i += RS_THREADS) {
            const int j = i / ss;
            s_g[j][i - j * ss] = grids[(long)n0 * ss + i];
        }
        if (tid < 2 * np) s_shift[tid >> 1][tid & 1] = shifts[2 * (long)n0 + tid];
        __syncthreads();
        if (live) {
            for (int j = 0; j < np; ++j) {
                int y0, y1, x0, x1;
                float ty, tx;
                at_source(y + s_shift[j][0], sy, s, y0, y1, ty);
                at_source(x + s_shift[j][1], sx, s, x0, x1, tx);
                const float m = rs_mask(s_g[j], s, y0, y1, ty, x0, x1, tx);
                at_fma_tile<RS_KT>(s_w[j], m, a);
            }
        }
    }
    if (live) at_store_acc<RS_KT>(acc, plane, p, k0, kt, a);
}

extern "C" int scouter_rise_accumulate_f32(const float* logp, const int* cols, const unsigned char* grids, const int* shifts,
                                           float* acc, int N, int n_classes, int K, int H, int W, int s, float scale,
                                           void* stream) {
    SC_REQUIRE(logp && cols && grids && shifts && acc,
               "rise_accumulate: null pointer (logp %p, cols %p, grids %p, shifts %p, acc %p)", (const void*)logp,
               (const void*)cols, (const void*)grids, (const void*)shifts, (void*)acc);
    SC_REQUIRE(N > 0 && n_classes > 0 && K > 0,
               "rise_accumulate: bad arguments (N %d, n_classes %d, K %d: each must be at least 1)", N, n_classes, K);
    if (int rc = rs_check_grid("rise_accumulate", H, W, s)) return rc;
    SC_REQUIRE(scale == scale, "rise_accumulate: scale is not a number");
    SC_REQUIRE((((uintptr_t)logp | (uintptr_t)cols | (uintptr_t)shifts | (uintptr_t)acc) & 3) == 0,
               "rise_accumulate: misaligned pointer (logp, cols, shifts and acc must be 4-byte aligned)");
    SC_UNSUPPORTED((long)H * W < (1L << 31), "rise_accumulate: map %d x %d is past the 32-bit offsets", H, W);
    const int ktiles = sc_cdiv(K, RS_KT);
    SC_UNSUPPORTED(ktiles <= 65535, "rise_accumulate: K = %d classes (at most %d)", K, 65535 * RS_KT);
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)H * W;
    ScProfScope prof("rise_accumulate", st, (double)N * px * ktiles * (14.0 + 2.0 * RS_KT),
                     8.0 * K * px + 4.0 * N * (double)n_classes);
    hipLaunchKernelGGL(rise_accumulate_kernel, dim3((unsigned)sc_cdiv((long)H * W, RS_THREADS), (unsigned)ktiles),
                       dim3(RS_THREADS), 0, st, logp, cols, grids, shifts, acc, N, n_classes, K, H, W, s, scale);
    return sc_check_launch("rise_accumulate");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(HM_THREADS) void heat_maps_kernel(const float* __restrict__ maps, unsigned char* __restrict__ out,
                                                               long plane, float min_level) {
    __shared__ float s_lo[HM_WAVES], s_hi[HM_WAVES];
    const int tid = threadIdx.x;
    const float* __restrict__ src = maps + (long)blockIdx.x * plane;

    // ---- the extrema of v = max(map, 0)
    float lo = INFINITY, hi = -INFINITY;
    for (long i = tid; i < plane; i += HM_THREADS) {
        const float v = fmaxf(src[i], 0.f);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    at_block_minmax<HM_WAVES>(lo, hi, s_lo, s_hi);

    // ---- the bytes
    const AtHeatScale scale(lo, hi, min_level);
    unsigned char* __restrict__ dst = out + (long)blockIdx.x * plane;
    for (long i = tid; i < plane; i += HM_THREADS) dst[i] = scale.byte(fmaxf(src[i], 0.f));
}

extern "C" int scouter_heat_maps_u8(const float* maps, unsigned char* out, int M, int H, int W, float min_level, void* stream) {
    SC_REQUIRE(maps && out, "heat_maps: null pointer (maps %p, out %p)", (const void*)maps, (void*)out);
    SC_REQUIRE(((uintptr_t)maps & 3) == 0, "heat_maps: misaligned pointer (maps must be 4-byte aligned)");
    SC_REQUIRE(M > 0 && H > 0 && W > 0, "heat_maps: bad arguments (M %d maps of %d x %d)", M, H, W);
    SC_REQUIRE(min_level == min_level, "heat_maps: min_level is not a number");
    SC_UNSUPPORTED((long)H * W < (1L << 31), "heat_maps: map %d x %d is past the 32-bit offsets", H, W);
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)M * H * W;
    ScProfScope prof("heat_maps", st, 8.0 * px, 9.0 * px);
    hipLaunchKernelGGL(heat_maps_kernel, dim3((unsigned)M), dim3(HM_THREADS), 0, st, maps, out, (long)H * W, min_level);
    return sc_check_launch("heat_maps");
}
