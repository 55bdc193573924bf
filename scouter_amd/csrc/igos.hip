// I-GOS (Qi, Khorram, Fuxin, AAAI 2020: integrated-gradient optimised saliency; what the reference's torchcam_vis.py runs first
// of all): the mask side of one iteration (tools/attribution.py igos).  R coarse masks pmask [R][hm][wm] in [0, 1] of ONE image
// [C][H][W] and its baseline, one mask per class.  No atomics, every cross-thread sum in one fixed order that depends on the
// shapes alone: two calls give the same bits, and a mask's values do not depend on the other masks of the call.
//
// U is the align-corners bilinear upsampler (torch.nn.UpsamplingBilinear2d): ig_source / at_bilerp of attr_common.h, the scales
// formed once on the host (ig_scale).  d = image - base is the fp32 difference, formed where it is used.
//
// igos_upsample_kernel: out[r] = U(pmask[r]).
// igos_path_kernel: stream row g = r S + j of the path, a = (j + 1) / S: out = fmaf(sigma, z, fmaf(a U(p_r), d, base)), z the
//   value of noise_images for (seed, sample0 + j, element) (ib_noise).  blockIdx.y is j: a thread forms the noise of its pixels
//   once per channel and writes it into every row of the chunk that has this j, so the R masks of an image share the Philox and
//   Box-Muller work.  sigma == 0: no noise is formed.
// igos_accumulate_kernel: acc[r][q] = fma(w_j, sum_c (double)dx[g][c][q] (double)d[c][q], acc[r][q]) over the rows g = r S + j of the
//   chunk in ascending j, the channel sum from 0 in ascending c, w_j = ((j + 1) / S) / S in fp64.  blockIdx.y is the mask row.
// igos_gather_kernel: dmask[r][cell] = (float)(sum_u acc[r][u] wy_u wx_u + d loss1 / d cell): one wave per cell, the pixels of the
//   window that can touch the cell taken lane, lane + 64, ... (row-major) by one fma each, then a butterfly; a pixel's weight
//   on the cell comes from ig_source itself (the lower index with 1 - t, the upper one with t), so the adjoint matches U bit for
//   bit in its coordinates.  Lane 0 adds the regulariser's derivative in fp64 and rounds once.
// igos_stats_kernel: stats[r] = (loss1(p_r), sum dmask_r^2 over the stored fp32 values), one workgroup per row (ig_loss1).
// igos_trial_kernel: stream row g = r T1 + k of the line search: out = fmaf(U(cand_k), d, base), cand_k = ig_candidate per cell.
// igos_step_kernel: one workgroup per row: tot_k = loss1(cand_k) + exp(logp) for every k in fp64 (ig_loss1, the workgroup's fixed
//   order), thread 0 takes the first k >= 1 with not (tot_k > tot_0 - alpha steps[k] sum dmask^2), else the last; the curves and
//   the l1 adjustment; then p = cand_chosen in place, every cell by the thread that owns it, after the last read of a neighbour.
#include "attr_common.h"

constexpr int IG_THREADS = 256, IG_WAVES = IG_THREADS / 64;
constexpr int IG_ROW_THREADS = 1024, IG_ROW_WAVES = IG_ROW_THREADS / 64;  // the per-row kernels (stats, step)
constexpr int IG_MAX_CELLS = 16384;           // hm wm: one workgroup walks a mask T1 times (112 x 112 is 12544)
constexpr int IG_MAX_LADDER = 64;             // T1

// the shapes every kernel here shares, with their refusals
static int ig_check_grid(const char* what, int R, int H, int W, int hm, int wm) {
    SC_REQUIRE(R > 0, "%s: R = %d mask rows (at least 1)", what, R);
    SC_REQUIRE(H >= 2 && W >= 2, "%s: an image of %d x %d pixels (each side at least 2)", what, H, W);
    SC_REQUIRE(hm >= 2 && hm <= H && wm >= 2 && wm <= W, "%s: a mask of %d x %d cells for %d x %d pixels (2 <= hm <= H, 2 <= wm <= W)",
               what, hm, wm, H, W);
    SC_UNSUPPORTED((long)hm * wm <= IG_MAX_CELLS, "%s: a mask of %d x %d cells (at most %d cells)", what, hm, wm, IG_MAX_CELLS);
    SC_UNSUPPORTED(R <= 65535, "%s: R = %d mask rows (at most 65535 per call)", what, R);
    SC_UNSUPPORTED((double)R * H * W < 2147483648.0, "%s: %d masks of %d x %d pixels are past the 32-bit offsets", what, R, H, W);
    return SC_OK;
}

// a chunk [first, first + n) of a stream of `total` rows of C x H x W elements
static int ig_check_chunk(const char* what, int first, int n, long total, int C, int H, int W) {
    SC_REQUIRE(C > 0 && n > 0, "%s: bad arguments (C %d, n %d: each must be at least 1)", what, C, n);
    SC_REQUIRE(first >= 0 && (long)first + n <= total, "%s: rows [%d, %ld) lie outside the stream of %ld rows", what, first,
               (long)first + n, total);
    SC_UNSUPPORTED((double)n * C * H * W < 2147483648.0, "%s: a chunk of %d x %d x %d x %d elements is past the 32-bit offsets", what,
                   n, C, H, W);
    return SC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(IG_THREADS) void igos_upsample_kernel(const float* __restrict__ pmask, float* __restrict__ out, int H,
                                                                   int W, int hm, int wm, float sy, float sx) {
    constexpr int V = VEC ? 4 : 1;
    const float* __restrict__ pm = pmask + (long)blockIdx.x * hm * wm;
    float* __restrict__ o = out + (long)blockIdx.x * H * W;
    const auto cell = [&](int i) { return pm[i]; };
    const int wq = W / V;                                                     // (VEC: W is a multiple of 4)
    const long items = (long)H * wq;
    for (long i = (long)blockIdx.y * IG_THREADS + threadIdx.x; i < items; i += (long)gridDim.y * IG_THREADS) {
        const int y = (int)(i / wq), x = (int)(i - (long)y * wq) * V;
        int y0, y1;
        float ty, v[V];
        ig_source(y, sy, hm, y0, y1, ty);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            int x0, x1;
            float tx;
            ig_source(x + e, sx, wm, x0, x1, tx);
            v[e] = ig_upsample_at(cell, wm, y0, y1, ty, x0, x1, tx);
        }
        if constexpr (VEC) *(f32x4*)(o + (long)y * W + x) = f32x4{v[0], v[1], v[2], v[3]};
        else o[(long)y * W + x] = v[0];
    }
}

extern "C" int scouter_igos_upsample_f32(const float* pmask, float* out, int R, int H, int W, int hm, int wm, void* stream) {
    SC_REQUIRE(pmask && out, "igos_upsample: null pointer (pmask %p, out %p)", (const void*)pmask, (void*)out);
    if (int rc = ig_check_grid("igos_upsample", R, H, W, hm, wm)) return rc;
    SC_REQUIRE((((uintptr_t)pmask | (uintptr_t)out) & 3) == 0, "igos_upsample: misaligned pointer (pmask and out must be 4-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, IG_THREADS, (uintptr_t)out);
    ScProfScope prof("igos_upsample", st, 12.0 * R * (double)H * W, 4.0 * R * ((double)H * W + (double)hm * wm));
    const dim3 grid((unsigned)R, px.tiles);
    const float sy = ig_scale(hm, H), sx = ig_scale(wm, W);
    if (px.vec) hipLaunchKernelGGL(igos_upsample_kernel<true>, grid, dim3(IG_THREADS), 0, st, pmask, out, H, W, hm, wm, sy, sx);
    else hipLaunchKernelGGL(igos_upsample_kernel<false>, grid, dim3(IG_THREADS), 0, st, pmask, out, H, W, hm, wm, sy, sx);
    return sc_check_launch("igos_upsample");
}

// ---------------------------------------------------------------------------------------------------------------------------
// V pixels of one row of the image from column x: their source columns, once per thread
template <int V>
struct IgColumns {
    int x0[V], x1[V];
    float tx[V];
    __device__ __forceinline__ IgColumns(int x, float sx, int wm) {
#pragma unroll
        for (int e = 0; e < V; ++e) ig_source(x + e, sx, wm, x0[e], x1[e], tx[e]);
    }
};

// image and baseline of V elements from flat index q -> the baseline b and the fp32 difference d (base null: zeros)
template <int V>
__device__ __forceinline__ void ig_difference(const float* __restrict__ image, const float* __restrict__ base, long q, float (&b)[V],
                                              float (&d)[V]) {
    float x[V];
    at_load<V>(image + q, x);
    if (base) at_load<V>(base + q, b);
#pragma unroll
    for (int e = 0; e < V; ++e) {
        if (!base) b[e] = 0.f;
        d[e] = x[e] - b[e];
    }
}

template <int V>
__device__ __forceinline__ void ig_store(float* __restrict__ p, const float (&v)[V]) {
    if constexpr (V == 4) *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]};
    else *p = v[0];
}

template <bool VEC>
__global__ __launch_bounds__(IG_THREADS) void igos_path_kernel(const float* __restrict__ image, const float* __restrict__ base,
                                                               const float* __restrict__ pmask, float* __restrict__ out, int first,
                                                               int n, int S, int C, int H, int W, int hm, int wm, float sy, float sx,
                                                               float sigma, unsigned seed_lo, unsigned seed_hi, int sample0) {
    constexpr int V = VEC ? 4 : 1;
    const int j = blockIdx.y;                                                 // the point of the path; its rows are g0, g0 + S, ...
    const long end = (long)first + n;
    const long g0 = (long)first + ((j - first % S) + S) % S;
    if (g0 >= end) return;
    const float a = (float)(j + 1) / (float)S;
    const long plane = (long)H * W;
    const int cells = hm * wm, wq = W / V;
    const long items = (long)H * wq;
    const bool noisy = sigma != 0.f;
    for (long i = (long)blockIdx.x * IG_THREADS + threadIdx.x; i < items; i += (long)gridDim.x * IG_THREADS) {
        const int y = (int)(i / wq), x = (int)(i - (long)y * wq) * V;
        const long p = (long)y * W + x;
        int y0, y1;
        float ty;
        ig_source(y, sy, hm, y0, y1, ty);
        const IgColumns<V> col(x, sx, wm);
        for (int c = 0; c < C; ++c) {
            float b[V], d[V], z[V];
            ig_difference<V>(image, base, c * plane + p, b, d);
            if (noisy) ib_noise<V>(c * plane + p, (unsigned)(sample0 + j), seed_lo, seed_hi, z);
            for (long g = g0; g < end; g += S) {
                const float* __restrict__ pm = pmask + (g / S) * cells;
                const auto cell = [&](int k) { return pm[k]; };
                float v[V];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    const float m = a * ig_upsample_at(cell, wm, y0, y1, ty, col.x0[e], col.x1[e], col.tx[e]);
                    const float xx = fmaf(m, d[e], b[e]);
                    v[e] = noisy ? fmaf(sigma, z[e], xx) : xx;
                }
                ig_store<V>(out + ((g - first) * C + c) * plane + p, v);
            }
        }
    }
}

extern "C" int scouter_igos_path_images_f32(const float* image, const float* base, const float* pmask, float* out, int first, int n,
                                            int R, int n_steps, int C, int H, int W, int hm, int wm, float sigma, int seed_lo,
                                            int seed_hi, int sample0, void* stream) {
    SC_REQUIRE(image && pmask && out, "igos_path_images: null pointer (image %p, pmask %p, out %p)", (const void*)image,
               (const void*)pmask, (void*)out);
    if (int rc = ig_check_grid("igos_path_images", R, H, W, hm, wm)) return rc;
    SC_REQUIRE(n_steps > 0, "igos_path_images: n_steps = %d (at least 1)", n_steps);
    SC_UNSUPPORTED(n_steps <= 65535 && (long)R * n_steps < (1L << 31), "igos_path_images: %d rows of %d path points (at most 65535 points, "
                   "2^31 stream rows)", R, n_steps);
    if (int rc = ig_check_chunk("igos_path_images", first, n, (long)R * n_steps, C, H, W)) return rc;
    SC_REQUIRE(sigma >= 0.f && sigma <= 3.0e38f, "igos_path_images: sigma = %g (it must be finite and not negative)", (double)sigma);
    SC_REQUIRE(sample0 >= 0 && (long)sample0 + n_steps < (1L << 31), "igos_path_images: samples [%d, %ld) lie outside [0, 2^31)", sample0,
               (long)sample0 + n_steps);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)base | (uintptr_t)pmask | (uintptr_t)out) & 3) == 0,
               "igos_path_images: misaligned pointer (image, base, pmask and out must be 4-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, IG_THREADS, (uintptr_t)image | (uintptr_t)base | (uintptr_t)out);
    const double elems = (double)C * H * W;
    ScProfScope prof("igos_path_images", st, (sigma != 0.f ? 60.0 * (n < n_steps ? n : n_steps) : 0.0) * elems + 16.0 * n * elems,
                     4.0 * ((double)n * elems + 2.0 * elems + (double)R * hm * wm));
    const dim3 grid(px.tiles, (unsigned)n_steps);
    const float sy = ig_scale(hm, H), sx = ig_scale(wm, W);
    if (px.vec)
        hipLaunchKernelGGL(igos_path_kernel<true>, grid, dim3(IG_THREADS), 0, st, image, base, pmask, out, first, n, n_steps, C, H, W,
                           hm, wm, sy, sx, sigma, (unsigned)seed_lo, (unsigned)seed_hi, sample0);
    else
        hipLaunchKernelGGL(igos_path_kernel<false>, grid, dim3(IG_THREADS), 0, st, image, base, pmask, out, first, n, n_steps, C, H, W,
                           hm, wm, sy, sx, sigma, (unsigned)seed_lo, (unsigned)seed_hi, sample0);
    return sc_check_launch("igos_path_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(IG_THREADS) void igos_accumulate_kernel(const float* __restrict__ image, const float* __restrict__ base,
                                                                     const float* __restrict__ dx, double* __restrict__ acc,
                                                                     int first, int n, int S, int C, int H, int W) {
    constexpr int V = VEC ? 4 : 1;
    const long plane = (long)H * W;
    const int r = first / S + (int)blockIdx.y;                                // the mask row; its points of the chunk are [jlo, jhi)
    const long lo = (long)r * S, end = (long)first + n;
    const int jlo = (int)(first > lo ? first - lo : 0), jhi = (int)(end < lo + S ? end - lo : S);
    const long items = plane / V;                                             // (VEC: W, so the plane, is a multiple of 4)
    for (long i = (long)blockIdx.x * IG_THREADS + threadIdx.x; i < items; i += (long)gridDim.x * IG_THREADS) {
        const long p = i * V;
        double a[V];
        at_load<V>(acc + r * plane + p, a);
        for (int j = jlo; j < jhi; ++j) {
            const float* __restrict__ g = dx + (lo + j - first) * C * plane + p;
            double s[V];
#pragma unroll
            for (int e = 0; e < V; ++e) s[e] = 0.0;
            for (int c = 0; c < C; ++c) {
                float b[V], d[V], gv[V];
                ig_difference<V>(image, base, c * plane + p, b, d);
                at_load<V, true>(g + c * plane, gv);
#pragma unroll
                for (int e = 0; e < V; ++e) s[e] = fma((double)gv[e], (double)d[e], s[e]);
            }
            const double w = ((double)(j + 1) / (double)S) / (double)S;
#pragma unroll
            for (int e = 0; e < V; ++e) a[e] = fma(w, s[e], a[e]);
        }
        at_store<V>(acc + r * plane + p, a);
    }
}

extern "C" int scouter_igos_accumulate_f64(const float* image, const float* base, const float* dx, double* acc, int first, int n, int R,
                                           int n_steps, int C, int H, int W, void* stream) {
    SC_REQUIRE(image && dx && acc, "igos_accumulate: null pointer (image %p, dx %p, acc %p)", (const void*)image, (const void*)dx,
               (void*)acc);
    SC_REQUIRE(R > 0 && H >= 2 && W >= 2, "igos_accumulate: bad arguments (R %d at least 1, H %d and W %d at least 2)", R, H, W);
    SC_REQUIRE(n_steps > 0, "igos_accumulate: n_steps = %d (at least 1)", n_steps);
    SC_UNSUPPORTED((long)R * n_steps < (1L << 31) && (double)R * H * W < 2147483648.0,
                   "igos_accumulate: %d rows of %d path points or of %d x %d pixels are past the 32-bit offsets", R, n_steps, H, W);
    if (int rc = ig_check_chunk("igos_accumulate", first, n, (long)R * n_steps, C, H, W)) return rc;
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)base | (uintptr_t)dx) & 3) == 0 && ((uintptr_t)acc & 7) == 0,
               "igos_accumulate: misaligned pointer (image, base and dx must be 4-byte aligned, acc 8-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    const int rows = (first + n - 1) / n_steps - first / n_steps + 1;         // the mask rows the chunk touches
    SC_UNSUPPORTED(rows <= 65535, "igos_accumulate: a chunk over %d mask rows (at most 65535)", rows);
    const AtPixelGrid px = at_pixel_grid(H, W, IG_THREADS, (uintptr_t)image | (uintptr_t)base | (uintptr_t)dx | (uintptr_t)acc);
    const double elems = (double)C * H * W;
    ScProfScope prof("igos_accumulate", st, 3.0 * n * elems, 4.0 * n * elems + 8.0 * n * elems + 16.0 * rows * (double)H * W);
    const dim3 grid(px.tiles, (unsigned)rows);
    if (px.vec)
        hipLaunchKernelGGL(igos_accumulate_kernel<true>, grid, dim3(IG_THREADS), 0, st, image, base, dx, acc, first, n, n_steps, C, H, W);
    else
        hipLaunchKernelGGL(igos_accumulate_kernel<false>, grid, dim3(IG_THREADS), 0, st, image, base, dx, acc, first, n, n_steps, C, H, W);
    return sc_check_launch("igos_accumulate");
}

// ---------------------------------------------------------------------------------------------------------------------------
// The regulariser loss1(p) = l1 mean|1 - p| + tv (mean|p[i,:] - p[i+1,:]|^beta + mean|p[:,j] - p[:,j+1]|^beta) of one mask,
// cell(i) its values, by a workgroup of THREADS threads: a thread adds its cells t, t + THREADS, ... in ascending order, the
// three sums meet by at_block_sum.  Valid in thread 0.  Ends after a barrier that FOLLOWS the last read of s_part, so the next
// call may reuse it.
template <int THREADS, typename Cell>
__device__ __forceinline__ double ig_loss1(Cell cell, int hm, int wm, double l1, double tv, double beta,
                                           double (*s_part)[THREADS / 64]) {
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const int cells = hm * wm;
    for (int i = threadIdx.x; i < cells; i += THREADS) {
        const int ci = i / wm, cj = i - ci * wm;
        const double p = (double)cell(i);
        s1 += fabs(1.0 - p);
        if (ci < hm - 1) s2 += pow(fabs(p - (double)cell(i + wm)), beta);
        if (cj < wm - 1) s3 += pow(fabs(p - (double)cell(i + 1)), beta);
    }
    const double t1 = at_block_sum<THREADS / 64>(s1, s_part[0]);
    const double t2 = at_block_sum<THREADS / 64>(s2, s_part[1]);
    const double t3 = at_block_sum<THREADS / 64>(s3, s_part[2]);
    __syncthreads();
    return l1 * (t1 / (double)cells) + tv * (t2 / ((double)(hm - 1) * wm) + t3 / ((double)hm * (wm - 1)));
}

// d |delta|^beta / d delta, 0 at delta = 0 (and for a NaN)
__device__ __forceinline__ double ig_tv_slope(double delta, double beta) {
    if (delta > 0.0) return beta * pow(delta, beta - 1.0);
    if (delta < 0.0) return -beta * pow(-delta, beta - 1.0);
    return 0.0;
}

__global__ __launch_bounds__(IG_THREADS) void igos_gather_kernel(const float* __restrict__ pmask, const double* __restrict__ acc,
                                                                 const float* __restrict__ l1, float* __restrict__ dmask,
                                                                 long cells_total, int H, int W, int hm, int wm, float sy, float sx,
                                                                 double tv, double beta) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * IG_WAVES + wv;                          // (uniform over the wave)
    if (c >= cells_total) return;
    const int cells = hm * wm;
    const int r = (int)(c / cells), cc = (int)(c - (long)r * cells);
    const int ci = cc / wm, cj = cc - ci * wm;
    // the pixels whose source coordinate lies inside (ci - 1, ci + 1), with two rows to spare on either side: whether a pixel
    // touches the cell is decided by ig_source alone
    const int ylo = max((int)((float)(ci - 1) / sy) - 2, 0), yhi = min((int)((float)(ci + 1) / sy) + 2, H - 1);
    const int xlo = max((int)((float)(cj - 1) / sx) - 2, 0), xhi = min((int)((float)(cj + 1) / sx) + 2, W - 1);
    const int nw = xhi - xlo + 1, nt = (yhi - ylo + 1) * nw;
    const double* __restrict__ a = acc + (long)r * H * W;
    double g = 0.0;
    for (int t = lane; t < nt; t += 64) {
        const int ly = t / nw, y = ylo + ly, x = xlo + (t - ly * nw);
        int i0, i1;
        float tt;
        ig_source(y, sy, hm, i0, i1, tt);
        const double wy = (i0 == ci ? 1.0 - (double)tt : 0.0) + (i1 == ci ? (double)tt : 0.0);
        ig_source(x, sx, wm, i0, i1, tt);
        const double wx = (i0 == cj ? 1.0 - (double)tt : 0.0) + (i1 == cj ? (double)tt : 0.0);
        const double w = wy * wx;
        if (w != 0.0) g = fma(a[(long)y * W + x], w, g);
    }
    g = wave_sum_d(g);
    if (lane == 0) {
        const float* __restrict__ pm = pmask + (long)r * cells;
        const double p = (double)pm[cc], one = 1.0 - p;
        double reg = (double)l1[r] * (one > 0.0 ? -1.0 : (one < 0.0 ? 1.0 : 0.0)) / (double)cells;
        double rows = 0.0, cols = 0.0;
        if (ci < hm - 1) rows += ig_tv_slope(p - (double)pm[cc + wm], beta);
        if (ci > 0) rows -= ig_tv_slope((double)pm[cc - wm] - p, beta);
        if (cj < wm - 1) cols += ig_tv_slope(p - (double)pm[cc + 1], beta);
        if (cj > 0) cols -= ig_tv_slope((double)pm[cc - 1] - p, beta);
        reg += tv * (rows / ((double)(hm - 1) * wm) + cols / ((double)hm * (wm - 1)));
        dmask[c] = (float)(g + reg);
    }
}

__global__ __launch_bounds__(IG_ROW_THREADS) void igos_stats_kernel(const float* __restrict__ pmask, const float* __restrict__ dmask,
                                                                    const float* __restrict__ l1, double* __restrict__ stats, int hm,
                                                                    int wm, double tv, double beta) {
    __shared__ double s_part[3][IG_ROW_WAVES], s_sq[IG_ROW_WAVES];
    const int r = blockIdx.x, cells = hm * wm;
    const float* __restrict__ pm = pmask + (long)r * cells;
    const float* __restrict__ dm = dmask + (long)r * cells;
    const double loss = ig_loss1<IG_ROW_THREADS>([&](int i) { return pm[i]; }, hm, wm, (double)l1[r], tv, beta, s_part);
    double q = 0.0;
    for (int i = threadIdx.x; i < cells; i += IG_ROW_THREADS) q = fma((double)dm[i], (double)dm[i], q);
    q = at_block_sum<IG_ROW_WAVES>(q, s_sq);
    if (threadIdx.x == 0) {
        stats[2 * r] = loss;
        stats[2 * r + 1] = q;
    }
}

static int ig_check_regulariser(const char* what, float tv_coeff, float tv_beta) {
    SC_REQUIRE(tv_coeff >= 0.f && tv_coeff <= 3.0e38f, "%s: tv_coeff = %g (it must be finite and not negative)", what, (double)tv_coeff);
    SC_REQUIRE(tv_beta >= 1.f && tv_beta <= 64.f, "%s: tv_beta = %g (it must lie inside [1, 64])", what, (double)tv_beta);
    return SC_OK;
}

extern "C" int scouter_igos_mask_grad_f32(const float* pmask, const double* acc, const float* l1, float* dmask, double* stats,
                                          float tv_coeff, float tv_beta, int R, int H, int W, int hm, int wm, void* stream) {
    SC_REQUIRE(pmask && acc && l1 && dmask && stats, "igos_mask_grad: null pointer (pmask %p, acc %p, l1 %p, dmask %p, stats %p)",
               (const void*)pmask, (const void*)acc, (const void*)l1, (void*)dmask, (void*)stats);
    if (int rc = ig_check_grid("igos_mask_grad", R, H, W, hm, wm)) return rc;
    if (int rc = ig_check_regulariser("igos_mask_grad", tv_coeff, tv_beta)) return rc;
    SC_REQUIRE((((uintptr_t)pmask | (uintptr_t)l1 | (uintptr_t)dmask) & 3) == 0 && (((uintptr_t)acc | (uintptr_t)stats) & 7) == 0,
               "igos_mask_grad: misaligned pointer (pmask, l1 and dmask must be 4-byte aligned, acc and stats 8-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    const long cells_total = (long)R * hm * wm;
    ScProfScope prof("igos_mask_grad", st, 40.0 * R * (double)H * W, 8.0 * R * (double)H * W + 12.0 * (double)cells_total);
    const float sy = ig_scale(hm, H), sx = ig_scale(wm, W);
    hipLaunchKernelGGL(igos_gather_kernel, dim3((unsigned)sc_cdiv(cells_total, IG_WAVES)), dim3(IG_THREADS), 0, st, pmask, acc, l1,
                       dmask, cells_total, H, W, hm, wm, sy, sx, (double)tv_coeff, (double)tv_beta);
    hipLaunchKernelGGL(igos_stats_kernel, dim3((unsigned)R), dim3(IG_ROW_THREADS), 0, st, pmask, dmask, l1, stats, hm, wm,
                       (double)tv_coeff, (double)tv_beta);
    return sc_check_launch("igos_mask_grad");
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(IG_THREADS) void igos_trial_kernel(const float* __restrict__ image, const float* __restrict__ base,
                                                                const float* __restrict__ pmask, const float* __restrict__ dmask,
                                                                const float* __restrict__ steps, float* __restrict__ out, int first,
                                                                int T1, int C, int H, int W, int hm, int wm, float sy, float sx) {
    constexpr int V = VEC ? 4 : 1;
    const long g = (long)first + blockIdx.y;
    const int r = (int)(g / T1), k = (int)(g - (long)r * T1);
    const float step = steps[k];
    const long plane = (long)H * W;
    const float* __restrict__ pm = pmask + (long)r * hm * wm;
    const float* __restrict__ dm = dmask + (long)r * hm * wm;
    const auto cell = [&](int i) { return ig_candidate(pm[i], dm[i], step); };
    float* __restrict__ o = out + (long)blockIdx.y * C * plane;
    const int wq = W / V;
    const long items = (long)H * wq;
    for (long i = (long)blockIdx.x * IG_THREADS + threadIdx.x; i < items; i += (long)gridDim.x * IG_THREADS) {
        const int y = (int)(i / wq), x = (int)(i - (long)y * wq) * V;
        const long p = (long)y * W + x;
        int y0, y1;
        float ty, u[V];
        ig_source(y, sy, hm, y0, y1, ty);
        const IgColumns<V> col(x, sx, wm);
#pragma unroll
        for (int e = 0; e < V; ++e) u[e] = ig_upsample_at(cell, wm, y0, y1, ty, col.x0[e], col.x1[e], col.tx[e]);
        for (int c = 0; c < C; ++c) {
            float b[V], d[V], v[V];
            ig_difference<V>(image, base, c * plane + p, b, d);
#pragma unroll
            for (int e = 0; e < V; ++e) v[e] = fmaf(u[e], d[e], b[e]);
            ig_store<V>(o + c * plane + p, v);
        }
    }
}

static int ig_check_ladder(const char* what, int T1) {
    SC_REQUIRE(T1 >= 2, "%s: a ladder of %d steps (steps[0] = 0 and at least one trial step)", what, T1);
    SC_UNSUPPORTED(T1 <= IG_MAX_LADDER, "%s: a ladder of %d steps (at most %d)", what, T1, IG_MAX_LADDER);
    return SC_OK;
}

extern "C" int scouter_igos_trial_images_f32(const float* image, const float* base, const float* pmask, const float* dmask,
                                             const float* steps, float* out, int first, int n, int R, int T1, int C, int H, int W,
                                             int hm, int wm, void* stream) {
    SC_REQUIRE(image && pmask && dmask && steps && out, "igos_trial_images: null pointer (image %p, pmask %p, dmask %p, steps %p, out %p)",
               (const void*)image, (const void*)pmask, (const void*)dmask, (const void*)steps, (void*)out);
    if (int rc = ig_check_grid("igos_trial_images", R, H, W, hm, wm)) return rc;
    if (int rc = ig_check_ladder("igos_trial_images", T1)) return rc;
    if (int rc = ig_check_chunk("igos_trial_images", first, n, (long)R * T1, C, H, W)) return rc;
    SC_UNSUPPORTED(n <= 65535, "igos_trial_images: n = %d rows (at most 65535 per call)", n);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)base | (uintptr_t)pmask | (uintptr_t)dmask | (uintptr_t)steps | (uintptr_t)out) & 3) == 0,
               "igos_trial_images: misaligned pointer (every array must be 4-byte aligned)");
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, IG_THREADS, (uintptr_t)image | (uintptr_t)base | (uintptr_t)out);
    const double elems = (double)C * H * W;
    ScProfScope prof("igos_trial_images", st, n * (20.0 * H * W + 3.0 * elems), 4.0 * ((double)n * elems + 2.0 * elems + 2.0 * R * hm * wm));
    const dim3 grid(px.tiles, (unsigned)n);
    const float sy = ig_scale(hm, H), sx = ig_scale(wm, W);
    if (px.vec)
        hipLaunchKernelGGL(igos_trial_kernel<true>, grid, dim3(IG_THREADS), 0, st, image, base, pmask, dmask, steps, out, first, T1, C,
                           H, W, hm, wm, sy, sx);
    else
        hipLaunchKernelGGL(igos_trial_kernel<false>, grid, dim3(IG_THREADS), 0, st, image, base, pmask, dmask, steps, out, first, T1, C,
                           H, W, hm, wm, sy, sx);
    return sc_check_launch("igos_trial_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IG_ROW_THREADS) void igos_step_kernel(float* __restrict__ pmask, const float* __restrict__ dmask,
                                                                   const float* __restrict__ steps, const float* __restrict__ logp,
                                                                   const int* __restrict__ cols, const double* __restrict__ stats,
                                                                   float* __restrict__ l1, double* __restrict__ curves, int T1,
                                                                   int n_out, int hm, int wm, int it, int n_iters, double alpha,
                                                                   double tv, double beta, int adapt) {
    __shared__ double s_part[3][IG_ROW_WAVES], s_tot[IG_MAX_LADDER], s_first[2];
    __shared__ int s_chosen;
    const int r = blockIdx.x, cells = hm * wm;
    float* __restrict__ pm = pmask + (long)r * cells;
    const float* __restrict__ dm = dmask + (long)r * cells;
    const float l1_now = l1[r];
    const int col = min(max(cols[r], 0), n_out - 1);                          // (the host refuses an index outside)
    for (int k = 0; k < T1; ++k) {
        const float step = steps[k];
        const double loss = ig_loss1<IG_ROW_THREADS>([&](int i) { return ig_candidate(pm[i], dm[i], step); }, hm, wm, (double)l1_now,
                                                     tv, beta, s_part);
        if (threadIdx.x == 0) {
            const double prob = exp((double)logp[((long)r * T1 + k) * n_out + col]);
            s_tot[k] = loss + prob;
            if (k == 0) { s_first[0] = loss; s_first[1] = prob; }
        }
    }
    if (threadIdx.x == 0) {
        int chosen = T1 - 1;
        for (int k = 1; k < T1; ++k) {
            const double thr = s_tot[0] - alpha * (double)steps[k] * stats[2 * r + 1];
            if (!(s_tot[k] > thr)) { chosen = k; break; }
        }
        double* __restrict__ cv = curves + ((long)r * n_iters + it) * 4;
        cv[0] = s_first[0];
        cv[1] = s_first[1];
        cv[2] = (double)steps[chosen];
        cv[3] = (double)chosen;
        if (adapt && n_iters > 3) {
            const double moved = fabs(s_first[1] - curves[(long)r * n_iters * 4 + 1]);   // (it == 0: the entry just written)
            if (it == n_iters / 2) {
                if (moved <= 1e-3) l1[r] = l1_now / 10.f;
            } else if (it == (int)((double)n_iters / 1.25)) {
                if (moved <= 1e-2) l1[r] = l1_now / 5.f;
            }
        }
        s_chosen = chosen;
    }
    __syncthreads();
    const float step = steps[s_chosen];
    for (int i = threadIdx.x; i < cells; i += IG_ROW_THREADS) pm[i] = ig_candidate(pm[i], dm[i], step);
}

extern "C" int scouter_igos_step_f32(float* pmask, const float* dmask, const float* steps, const float* logp, const int* cols,
                                     const double* stats, float* l1, double* curves, int R, int T1, int n_out, int hm, int wm, int it,
                                     int n_iters, double alpha, float tv_coeff, float tv_beta, int adapt, void* stream) {
    SC_REQUIRE(pmask && dmask && steps && logp && cols && stats && l1 && curves,
               "igos_step: null pointer (pmask %p, dmask %p, steps %p, logp %p, cols %p, stats %p, l1 %p, curves %p)", (void*)pmask,
               (const void*)dmask, (const void*)steps, (const void*)logp, (const void*)cols, (const void*)stats, (void*)l1, (void*)curves);
    SC_REQUIRE(R > 0 && n_out > 0, "igos_step: bad arguments (R %d, n_out %d: each must be at least 1)", R, n_out);
    SC_REQUIRE(hm >= 2 && wm >= 2, "igos_step: a mask of %d x %d cells (each side at least 2)", hm, wm);
    SC_UNSUPPORTED((long)hm * wm <= IG_MAX_CELLS, "igos_step: a mask of %d x %d cells (at most %d cells)", hm, wm, IG_MAX_CELLS);
    SC_UNSUPPORTED(R <= 65535, "igos_step: R = %d mask rows (at most 65535 per call)", R);
    if (int rc = ig_check_ladder("igos_step", T1)) return rc;
    if (int rc = ig_check_regulariser("igos_step", tv_coeff, tv_beta)) return rc;
    SC_REQUIRE(it >= 0 && it < n_iters, "igos_step: iteration %d lies outside [0, n_iters = %d)", it, n_iters);
    SC_REQUIRE(alpha >= 0.0 && alpha <= 1.0e300, "igos_step: alpha = %g (it must be finite and not negative)", alpha);
    SC_REQUIRE(adapt == 0 || adapt == 1, "igos_step: adapt = %d (0 or 1)", adapt);
    SC_REQUIRE((((uintptr_t)pmask | (uintptr_t)dmask | (uintptr_t)steps | (uintptr_t)logp | (uintptr_t)cols | (uintptr_t)l1) & 3) == 0 &&
                   (((uintptr_t)stats | (uintptr_t)curves) & 7) == 0,
               "igos_step: misaligned pointer (stats and curves must be 8-byte aligned, every other array 4-byte aligned)");
    SC_UNSUPPORTED((double)R * T1 * n_out < 2147483648.0 && (double)R * n_iters * 4 < 2147483648.0,
                   "igos_step: %d x %d rows of %d outputs or %d iterations are past the 32-bit offsets", R, T1, n_out, n_iters);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("igos_step", st, 60.0 * R * T1 * (double)hm * wm, 4.0 * R * (3.0 * hm * wm + T1));
    hipLaunchKernelGGL(igos_step_kernel, dim3((unsigned)R), dim3(IG_ROW_THREADS), 0, st, pmask, dmask, steps, logp, cols, stats, l1, curves,
                       T1, n_out, hm, wm, it, n_iters, alpha, (double)tv_coeff, (double)tv_beta, adapt);
    return sc_check_launch("igos_step");
}
