// Hamilton-Adams demosaic of packed raw frames (green plane, then red / blue) and its inverse, the re-mosaic of an RGB frame.
// Compiled with -ffp-contract=off: the demosaic has hard sign() selections (util/Hamilton_Adam_demo.py:138-139,168-169), so
// the arithmetic is kept operation for operation as the reference's ATen ops evaluate it.  The stencils are in demosaic.h.
#include "demosaic.h"

namespace {

// rbs = floats from one sequence's raw frame to the next one's (4hw when dense; more for a channel slice of a wider tensor)
template <int PH>
__global__ void ha_green_kernel(const float* __restrict__ raw, float* __restrict__ green, int n, int h,
                                int w, int64_t rbs) {
    const int H = 2 * h, W = 2 * w;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * H * W) return;
    const int x = idx % W;
    const int y = (idx / W) % H;
    const int b = idx / ((size_t)W * H);
    Cfa c{raw + (size_t)b * rbs, h, w, H, W};
    green[idx] = ha_green_at<PH>(c, y, x);
}

template <int PH>
__global__ void ha_rb_kernel(const float* __restrict__ raw, const float* __restrict__ green,
                             float* __restrict__ out, int n, int h, int w, int64_t bstride, int pstride,
                             int cstride, int64_t rbs) {
    const int H = 2 * h, W = 2 * w;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)n * H * W) return;
    const int x = idx % W;
    const int y = (idx / W) % H;
    const int b = idx / ((size_t)W * H);
    Cfa c{raw + (size_t)b * rbs, h, w, H, W};
    const float* gp = green + (size_t)b * H * W;
    Ring q;
    load_ring<PH>(c, gp, H, W, y, x, q);
    const float g0 = q.g[1][1];
    float rb[2];
    ha_red_blue<PH>(q, y, x, rb);
    float* o = out + (size_t)b * bstride + ((size_t)y * W + x) * pstride;
    o[0] = rb[0];
    o[cstride] = g0;
    o[2 * (size_t)cstride] = rb[1];
}

// HamiltonAdam.remosaick from the NHWC4 previous output: the packed planes [B][4][H/2][W/2] of the pattern, channel c =
// CFA position (c >> 1, c & 1) holding the colour of its site c ^ PH -- the inverse of the packing, so remosaick(HA(raw)) is
// raw for every pattern.  For GBRG (util/Hamilton_Adam_demo.py:237-246): G(even row, even col), B(even, odd), R(odd, even),
// G(odd, odd).  Pure indexing.
template <int PH>
__global__ void remosaick4_kernel(const float* __restrict__ rgb4, float* __restrict__ raw, int B, int H, int W) {
    const int h = H / 2, w = W / 2;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * 4 * h * w) return;
    const int x = idx % w;
    const int y = (idx / w) % h;
    const int c = (idx / ((size_t)w * h)) % 4;
    const int b = idx / ((size_t)4 * w * h);
    const int yy = 2 * y + (c >> 1), xx = 2 * x + (c & 1);
    const int site = c ^ PH;
    const int ch = site == 0 || site == 3 ? 1 : (site == 1 ? 2 : 0);
    raw[idx] = rgb4[(((size_t)b * H + yy) * W + xx) * 4 + ch];
}

}  // namespace

hipError_t launch_ha_green(const float* raw, float* green, int n, int h, int w, int64_t rbs, hipStream_t s, int bayer) {
    RVDD_BAYER_DISPATCH(bayer, ha_green_kernel, dim3(nblocks((size_t)n * 4 * h * w, 256)), dim3(256), 0, s, raw, green, n, h, w, rbs);
    return hipGetLastError();
}

hipError_t launch_demosaic(const float* raw, float* green_scratch, float* out, int n, int h, int w,
                           int64_t bstride, int pstride, int cstride, hipStream_t s, int64_t raw_bstride, int bayer) {
    const size_t npix = (size_t)n * 4 * h * w;
    if (!npix) return hipSuccess;
    const int64_t rbs = raw_bstride ? raw_bstride : (int64_t)4 * h * w;
    RVDD_BAYER_DISPATCH(bayer, ha_green_kernel, dim3(nblocks(npix, 256)), dim3(256), 0, s, raw, green_scratch, n, h, w, rbs);
    RVDD_BAYER_DISPATCH(bayer, ha_rb_kernel, dim3(nblocks(npix, 256)), dim3(256), 0, s, raw, green_scratch, out, n, h,
                        w, bstride, pstride, cstride, rbs);
    return hipGetLastError();
}

hipError_t launch_remosaick4(const float* rgb4, float* raw, int B, int H, int W, hipStream_t s, int bayer) {
    const size_t n = (size_t)B * H * W;
    if (!n) return hipSuccess;
    RVDD_BAYER_DISPATCH(bayer, remosaick4_kernel, dim3(nblocks(n, 256)), dim3(256), 0, s, rgb4, raw, B, H, W);
    return hipGetLastError();
}
