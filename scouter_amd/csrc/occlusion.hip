// Occlusion sensitivity (Zeiler & Fergus, ECCV 2014; captum's Occlusion): a window slides over the image, every occluded copy goes
// through the model, and a pixel's score is the mean, over the windows that covered it, of what the class lost.  Two kernels, each
// with one fixed order per output element and no atomics, so two calls give the same bits.
//
// The geometry, per axis of `size` pixels with window `win` and stride `str`, 1 <= str <= win <= size (oc_count, oc_first):
//   n = 1 + ceil((size - win) / str) windows; window i covers [i str, min(i str + win, size)) -- the last one may be partial;
//   the windows that cover pixel y are i in [max(0, ceil((y - win + 1) / str)), min(n - 1, floor(y / str))], never an empty range.
// Window n = iy nx + ix, N = ny nx.
//
// occlude_images_kernel: row 0 of out is the image, row 1 + j the image with window first + j set to `fill` in every channel -- a
//   select, every other value an exact copy.  A workgroup belongs to ONE row (blockIdx.x); it reads the image (L2-resident after
//   the first row) and writes its row once: the kernel is HBM stores.  W a multiple of 4 and 16-byte aligned pointers: four
//   pixels of a row per thread, 16-byte loads and stores; anything else: one pixel per thread.  The same bits either way.
// occlusion_finish_kernel: out[k][y][x] = (float)(sum of deltas[k][iy nx + ix] over the covering windows / their number), the sum
//   in fp64 with iy ascending, then ix ascending; one thread per output element.
#include "attr_common.h"

constexpr int OC_THREADS = 256;

struct OcGeometry {
    int H, W, wh, ww, sy, sx, ny, nx;
};

// the number of windows of one axis
static inline int oc_count(int size, int win, int str) { return 1 + (size - win + str - 1) / str; }

// the first window that covers pixel y: max(0, ceil((y - win + 1) / str))
__device__ __forceinline__ int oc_first(int y, int win, int str) { return y - win + 1 <= 0 ? 0 : (y - win + str) / str; }

// the geometry every call of the family refuses; fills g
static int oc_check_geometry(const char* what, int H, int W, int wh, int ww, int sy, int sx, OcGeometry& g) {
    SC_REQUIRE(H > 0 && W > 0, "%s: bad arguments (H %d, W %d: each must be at least 1)", what, H, W);
    SC_REQUIRE(sy >= 1 && sy <= wh && wh <= H, "%s: rows: stride %d, window %d, size %d (1 <= stride <= window <= size)", what, sy,
               wh, H);
    SC_REQUIRE(sx >= 1 && sx <= ww && ww <= W, "%s: columns: stride %d, window %d, size %d (1 <= stride <= window <= size)", what,
               sx, ww, W);
    SC_UNSUPPORTED((long)H * W < (1L << 31), "%s: map %d x %d is past the 32-bit offsets", what, H, W);
    g = OcGeometry{H, W, wh, ww, sy, sx, oc_count(H, wh, sy), oc_count(W, ww, sx)};      // (ny nx <= H W < 2^31)
    return SC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(OC_THREADS) void occlude_images_kernel(const float* __restrict__ image, float* __restrict__ out,
                                                                    int first, int C, OcGeometry g, float fill) {
    const int r = blockIdx.x, tid = threadIdx.x;
    int y_lo = 0, y_hi = 0, x_lo = 0, x_hi = 0;                 // (row 0, the image itself: an empty window)
    if (r > 0) {                                                // (the host keeps 0 <= first and first + n <= ny nx)
        const int n = first + r - 1, iy = n / g.nx, ix = n - iy * g.nx;
        y_lo = iy * g.sy; y_hi = min(y_lo + g.wh, g.H);
        x_lo = ix * g.sx; x_hi = min(x_lo + g.ww, g.W);
    }
    const long plane = (long)g.H * g.W;
    float* __restrict__ o = out + (long)r * C * plane;
    constexpr int V = VEC ? 4 : 1;
    const int wq = g.W / V;                                     // (VEC: W is a multiple of 4)
    const long items = (long)g.H * wq;
    for (long i = (long)blockIdx.y * OC_THREADS + tid; i < items; i += (long)gridDim.y * OC_THREADS) {
        const int y = (int)(i / wq), x = (int)(i - (long)y * wq) * V;
        const long p = (long)y * g.W + x;
        const bool in_rows = y >= y_lo && y < y_hi;
        bool hide[V];
#pragma unroll
        for (int k = 0; k < V; ++k) hide[k] = in_rows && x + k >= x_lo && x + k < x_hi;
        for (int c = 0; c < C; ++c) {
            float v[V];
            at_load<V>(image + c * plane + p, v);
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = hide[k] ? fill : v[k];
            if constexpr (VEC) *(f32x4*)(o + c * plane + p) = f32x4{v[0], v[1], v[2], v[3]};
            else o[c * plane + p] = v[0];
        }
    }
}

extern "C" int scouter_occlude_images_f32(const float* image, float* out, int first, int n, int C, int H, int W, int wh, int ww,
                                          int sy, int sx, float fill, void* stream) {
    SC_REQUIRE(image && out, "occlude_images: null pointer (image %p, out %p)", (const void*)image, (void*)out);
    SC_REQUIRE((((uintptr_t)image | (uintptr_t)out) & 3) == 0,
               "occlude_images: misaligned pointer (image and out must be 4-byte aligned)");
    SC_REQUIRE(n > 0 && C > 0, "occlude_images: bad arguments (n %d, C %d: each must be at least 1)", n, C);
    OcGeometry g;
    if (int rc = oc_check_geometry("occlude_images", H, W, wh, ww, sy, sx, g)) return rc;
    const long N = (long)g.ny * g.nx;
    SC_REQUIRE(first >= 0 && (long)first + n <= N, "occlude_images: windows [%d, %ld) lie outside [0, ny nx = %d x %d = %ld)", first,
               (long)first + n, g.ny, g.nx, N);
    SC_REQUIRE(fill == fill, "occlude_images: fill is not a number");
    SC_UNSUPPORTED((long)C * H * W < (1L << 31), "occlude_images: image of %d x %d x %d elements is past the 32-bit offsets", C, H,
                   W);
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(H, W, OC_THREADS, (uintptr_t)image | (uintptr_t)out);
    const double elems = (1.0 + n) * C * H * W;
    ScProfScope prof("occlude_images", st, elems, 4.0 * (elems + (double)C * H * W));
    const dim3 grid((unsigned)(1 + n), px.tiles);
    if (px.vec) hipLaunchKernelGGL(occlude_images_kernel<true>, grid, dim3(OC_THREADS), 0, st, image, out, first, C, g, fill);
    else hipLaunchKernelGGL(occlude_images_kernel<false>, grid, dim3(OC_THREADS), 0, st, image, out, first, C, g, fill);
    return sc_check_launch("occlude_images");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OC_THREADS) void occlusion_finish_kernel(const double* __restrict__ deltas, float* __restrict__ out,
                                                                      long total, OcGeometry g) {
    const long i = (long)blockIdx.x * OC_THREADS + threadIdx.x;
    if (i >= total) return;
    const long plane = (long)g.H * g.W;
    const int k = (int)(i / plane), p = (int)(i - (long)k * plane);
    const int y = p / g.W, x = p - y * g.W;
    const int iy0 = oc_first(y, g.wh, g.sy), iy1 = min(g.ny - 1, y / g.sy);
    const int ix0 = oc_first(x, g.ww, g.sx), ix1 = min(g.nx - 1, x / g.sx);
    const double* __restrict__ d = deltas + (long)k * g.ny * g.nx;
    double s = 0.0;
    for (int iy = iy0; iy <= iy1; ++iy)
        for (int ix = ix0; ix <= ix1; ++ix) s += d[(long)iy * g.nx + ix];
    const int count = (iy1 - iy0 + 1) * (ix1 - ix0 + 1);       // (at least 1: neither range is empty)
    out[i] = (float)(s / (double)count);
}

extern "C" int scouter_occlusion_finish_f32(const double* deltas, float* out, int K, int H, int W, int wh, int ww, int sy, int sx,
                                            void* stream) {
    SC_REQUIRE(deltas && out, "occlusion_finish: null pointer (deltas %p, out %p)", (const void*)deltas, (void*)out);
    SC_REQUIRE(((uintptr_t)deltas & 7) == 0 && ((uintptr_t)out & 3) == 0,
               "occlusion_finish: misaligned pointer (deltas must be 8-byte, out 4-byte aligned)");
    SC_REQUIRE(K > 0, "occlusion_finish: bad arguments (K %d must be at least 1)", K);
    OcGeometry g;
    if (int rc = oc_check_geometry("occlusion_finish", H, W, wh, ww, sy, sx, g)) return rc;
    const long total = (long)K * H * W;
    SC_UNSUPPORTED(total < (1L << 38), "occlusion_finish: %d maps of %d x %d are more than the grid holds", K, H, W);
    hipStream_t st = (hipStream_t)stream;
    const double windows = (double)sc_cdiv(wh, sy) * sc_cdiv(ww, sx);
    ScProfScope prof("occlusion_finish", st, (double)total * (windows + 1.0), (double)total * 4.0 + 8.0 * K * g.ny * (double)g.nx);
    hipLaunchKernelGGL(occlusion_finish_kernel, dim3((unsigned)sc_cdiv(total, OC_THREADS)), dim3(OC_THREADS), 0, st, deltas, out,
                       total, g);
    return sc_check_launch("occlusion_finish");
}
