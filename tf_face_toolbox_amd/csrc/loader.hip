// loader.hip -- the GPU transform of the input pipeline for gfx950 (include/fte.h "fte_preprocess_u8*", "fte_pack_gather_slots"):
// decoded uint8 images + the workers' draws in, the float32 NHWC batch out, bit for bit what tf_face_toolbox_amd/_decode_worker.py
// and preprocessing.py compute on the host.  The header decode, the bilinear tap and the colour tail are written ONCE (the zero-outside
// warp twice: see the aligned kernel), all under `#pragma clang fp contract(off)`:
// every product and sum rounds on its own, as numpy's do (hipcc's default would fuse them into FMAs; the __fmul_rn / __fadd_rn
// intrinsics are inline operators that carry the translation unit's contraction flag with them).  Wave = 64 lanes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "loader.h"

namespace {

// One slot per image: a header of int32 words, then the h0 x w0 x C bytes of the decoded image (mode 0) or the finished float32
// crop (mode 1: an image that did not fit its slot was transformed by the worker, every augmentation included).
// fte.h's words: 0 mode, 1 h0, 2 w0, 3 y0, 4 x0, 5 flip, 6 flags, 7..9 delta_b delta_h factor, 10 th, 11 tw, 12 rnd, 16..21 m.
// flags: 1 brightness, 2 hue, 4 saturation, 8 zoom, 16 affine.  Words 16..21 exist in aligned slots (128-byte header) only; the
// aligned kernel below reads them, and keeps its own decode.  Of words 0..12 a kernel uses the fields its entry documents and no
// others: the rest are dead loads inside the header, which the compiler drops.
constexpr int HEADER = 64, ALIGN_HEADER = 128;

struct SlotHeader {
    int mode, h0, w0, y0, x0, flip, flags;
    const float* colour;          // words 7..9 in place: delta_b, delta_h, factor.  colour_store fetches each under its flag's branch: a wave that
                                  // waits for them with the words above measured 4 % slower in the colour transform (profiles/loader_refactor.md)
    int th, tw, rnd;
};

__device__ __forceinline__ SlotHeader read_header(const unsigned char* slot) {
    const int* w = reinterpret_cast<const int*>(slot);
    SlotHeader h;
    h.mode = w[0]; h.h0 = w[1]; h.w0 = w[2]; h.y0 = w[3]; h.x0 = w[4]; h.flip = w[5]; h.flags = w[6];
    h.colour = reinterpret_cast<const float*>(w + 7);
    h.th = w[10]; h.tw = w[11]; h.rnd = w[12];
    return h;
}

// a source element as the float the host works on: a byte is scaled by 1/255 (convert_image_dtype), a plane's float is itself
__device__ __forceinline__ float texel(const unsigned char* p) {
#pragma clang fp contract(off)
    return (float)*p * (float)(1.0 / 255.0);
}
__device__ __forceinline__ float texel(const float* p) { return *p; }

// Pixel (yy, xx) of tf.image.resize_images(src [sh, sw, C], [dh, dw]) with ry = (float)sh / (float)dh, rx likewise (data.py:206-223
// of the reference; resize_window on the host).  TF-1.x ResizeBilinear, align_corners = False: in = out * (n_in / n_out),
// low = floor(in), high = min(low + 1, n_in - 1); the two neighbours of a row are blended along x, then the two rows along y.
// `low` is clamped into [0, n_in - 1] as well: for the headers the host writes the clamp never fires, for any other it keeps the
// four taps inside the h0 x w0 image (words 10..12 of a geometric slot steer sh, sw of the plane stages and are not trusted).
template <int C, class T>
__device__ __forceinline__ void bilinear_tap(const T* src, int sh, int sw, float ry, float rx, int yy, int xx, float* v) {
#pragma clang fp contract(off)
    const float py = (float)yy * ry, pxs = (float)xx * rx;
    const int ylo = min(max((int)floorf(py), 0), sh - 1), xlo = min(max((int)floorf(pxs), 0), sw - 1);
    const int yhi = min(ylo + 1, sh - 1), xhi = min(xlo + 1, sw - 1);
    const float yw = py - (float)ylo, xw = pxs - (float)xlo;
    const T* tl = src + ((long)ylo * sw + xlo) * C;
    const T* tr = src + ((long)ylo * sw + xhi) * C;
    const T* bl = src + ((long)yhi * sw + xlo) * C;
    const T* br = src + ((long)yhi * sw + xhi) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float a = texel(tl + c), b = texel(tr + c), d = texel(bl + c), e = texel(br + c);
        const float top = (b - a) * xw + a;
        const float bot = (e - d) * xw + d;
        v[c] = (bot - top) * yw + top;
    }
}

// The colour augmentation of preprocessing.py:22-38 of the reference (adjust_brightness, adjust_hue, adjust_saturation as
// tf_face_toolbox_amd/preprocessing.py restates them in float32), from the worker's draws in the slot header.  The draws only
// steer arithmetic, never an address.
//
// numpy's `%` on floats is floor-mod: m = fmod(a, b); m != 0 and of the other sign than b -> m + b (one rounded add);
// m == 0 -> +0 for b > 0.  The three uses below, on values the clip to [0, 1] bounds, without fmodf:
//   x % 6, x = (g - b) / dz in [-1, 1] and never -0 (g - b is +0 when g == b): fmod(x, 6) = x, so x < 0 ? x + 6 : x;
//   a % 1, any finite a: a >= 0: fmod = a - trunc(a) = a - floor(a), exact; a < 0: fl(fmod + 1) = fl(a - trunc(a) + 1)
//          = fl(a - floor(a)), the same single rounding (a negative integer gives +0 both ways): a - floorf(a);
//   t % 2, t = 6 h in [0, 6]: t - 2 floor(t / 2), every step exact.
__device__ __forceinline__ void aug_rgb_to_hsv(float r, float g, float b, float& h, float& s, float& mx) {
#pragma clang fp contract(off)
    mx = fmaxf(fmaxf(r, g), b);
    const float mn = fminf(fminf(r, g), b);
    const float d = mx - mn;
    s = mx > 0.f ? d / mx : 0.f;
    const float dz = d > 0.f ? d : 1.f;
    const float x = (mx == r ? g - b : mx == g ? b - r : r - g) / dz;      // one divide for the three branches: the same quotient
    float hh = mx == r ? (x < 0.f ? x + 6.f : x) : mx == g ? x + 2.f : x + 4.f;
    hh = hh / 6.0f;
    h = d > 0.f ? hh : 0.f;
}

__device__ __forceinline__ void aug_hsv_to_rgb(float h, float s, float v, float& r, float& g, float& b) {
#pragma clang fp contract(off)
    const float h6 = h * 6.0f;
    const float c = v * s;
    const float t = h6 - 2.f * floorf(h6 * 0.5f);
    const float x = c * (1.f - fabsf(t - 1.f));
    int i = (int)floorf(h6) % 6;                  // h can round to exactly 1.0 (a tiny negative sum + 1): sextant 6 % 6 = 0
    if (i < 0) i += 6;
    const float m = v - c;
    r = ((i == 0 || i == 5) ? c : (i == 1 || i == 4) ? x : 0.f) + m;
    g = ((i == 1 || i == 2) ? c : (i == 0 || i == 3) ? x : 0.f) + m;
    b = ((i == 3 || i == 4) ? c : (i == 2 || i == 5) ? x : 0.f) + m;
}

// the tail of every transform: COLOUR -> brightness / hue / saturation of one pixel by the header's flag bits; then (x - 0.5) / 0.5
template <int C, bool COLOUR>
__device__ __forceinline__ void colour_store(float* v, int flags, const float* colour, float* o) {
#pragma clang fp contract(off)
    if constexpr (COLOUR) {
        if (flags & 1) {                           // adjust_brightness(image, -delta): no clip of its own
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = v[c] - colour[0];
        }
        if constexpr (C == 3) {
            if (flags & 2) {                       // adjust_hue(clip(image, 0, 1), -delta)
                float h, sa, va;
                aug_rgb_to_hsv(fminf(fmaxf(v[0], 0.f), 1.f), fminf(fmaxf(v[1], 0.f), 1.f), fminf(fmaxf(v[2], 0.f), 1.f), h, sa, va);
                const float a = h + (-colour[1]);
                h = a - floorf(a);
                aug_hsv_to_rgb(h, sa, va, v[0], v[1], v[2]);
            }
            if (flags & 4) {                       // adjust_saturation(clip(image, 0, 1), factor): a second round trip, as on the host
                float h, sa, va;
                aug_rgb_to_hsv(fminf(fmaxf(v[0], 0.f), 1.f), fminf(fmaxf(v[1], 0.f), 1.f), fminf(fmaxf(v[2], 0.f), 1.f), h, sa, va);
                sa = fminf(fmaxf(sa * colour[2], 0.f), 1.f);
                aug_hsv_to_rgb(h, sa, va, v[0], v[1], v[2]);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (v[c] - 0.5f) / 0.5f;
}

// pixel px of a mode-1 slot: the worker's finished float32 crop, copied; a crop larger than the slot reads zeros past its end
template <int C>
__device__ __forceinline__ void copy_finished(const unsigned char* slot, int header, long slot_stride, long px, float* o) {
    const float* f = reinterpret_cast<const float*>(slot + header) + px * C;
    const bool fits = (px + 1) * C * (long)sizeof(float) <= slot_stride - header;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = fits ? f[c] : 0.f;
}

// ------------------------------------------------------------------------------------------------
// The two RESIZE entries, one thread per output pixel (fte_preprocess_u8, _aug): convert_image_dtype + resize_images + random_crop +
// random_flip_left_right + (x - 0.5) / 0.5 on a 64-byte header and the decoded h0 x w0 image: bilinear_tap at (y0 + r, x0 + col) of
// the in_h x in_w resized image, flip (of the OUTPUT column), colour (COLOUR: header words 6..9; the plain instantiation holds no
// colour code and reads no colour word) and normalise.
template <int C, bool COLOUR>
__global__ __launch_bounds__(256) void preprocess_pixel_kernel(const unsigned char* __restrict__ slots, float* __restrict__ out, long slot_stride,
                                                                int in_h, int in_w, int crop_h, int crop_w) {
#pragma clang fp contract(off)
    const int img = blockIdx.y;
    const unsigned char* slot = slots + (long)img * slot_stride;
    const SlotHeader hd = read_header(slot);
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= crop_h * crop_w) return;
    float* o = out + ((long)img * crop_h * crop_w + px) * C;
    if (hd.mode == 1) {
        copy_finished<C>(slot, HEADER, slot_stride, px, o);
        return;
    }
    const int r = px / crop_w, cc = px - r * crop_w;
    const int col = hd.flip ? crop_w - 1 - cc : cc;
    float v[C];
    bilinear_tap<C>(slot + HEADER, hd.h0, hd.w0, (float)hd.h0 / (float)in_h, (float)hd.w0 / (float)in_w, hd.y0 + r, hd.x0 + col, v);
    colour_store<C, COLOUR>(v, hd.flags, hd.colour, o);
}

// the channel dispatch of the one-thread-per-pixel kernels (grid: blocks of 256 pixels x images)
template <class K3, class K1, class... Args>
hipError_t launch_pixel(K3 k3, K1 k1, int n, int channels, int crop_h, int crop_w, hipStream_t st, Args... args) {
    const dim3 grid((crop_h * crop_w + 255) / 256, n);
    if (channels == 3) k3<<<grid, 256, 0, st>>>(args...);
    else k1<<<grid, 256, 0, st>>>(args...);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// five-point alignment in place of the resize (tf_face_toolbox_amd/preprocessing.py: align_window, align_warp): the worker
// hands over a WINDOW of the decoded image -- the part the aligned in_h x in_w image can read -- and the inverse similarity
// relative to that window's corner; the crop of the aligned image is warped straight from the window's bytes, then flipped,
// coloured (words 6..9: colour_store) and normalised.  Slot: a 128-byte header -- int32 words 0..15 as
// above with h0, w0 = the window's shape, words 16..21 = float32 bits of (a0, a1, a2, b0, b1, b2) -- then h0 x w0 x C bytes
// (mode 0) or the finished float32 crop (mode 1).  The warp is the AFFINE stage's formula on the window: output pixel (x, y) of
// the aligned image reads (sx, sy) = ((a0 x + a1 y) + a2, (b0 x + b1 y) + b2), zero outside the window; a pixel none of whose
// four taps lies inside is 0 (what the formula gives for finite coordinates; it settles the others).
//
// One thread per output pixel like preprocess_pixel_kernel, not one workgroup per image like the geometric kernel: nothing is
// staged and a pixel's 4 taps of C bytes are its only reads, so the simplest mapping was taken.  Neighbouring lanes' taps are
// (a0, b0) source pixels apart: how many window rows, i.e. cache lines, a wave's 64 pixels touch grows with |b0| (rotation x
// scale) -- two rows for an upright face, about 30 at (a0, b0) = (1.72, 0.46).  The launch measured 3x the plain resize's at that
// matrix (profiles/align_loader.md); which part of the kernel carries the factor was not measured and the mapping is not tuned.
// Words 16..21, h0 and w0 steer addresses and are not trusted: a tap is inside only if its FLOAT coordinates lie in
// [0, w0 - 1] x [0, h0 - 1] (false for a NaN), decided before any conversion to int; the float is clamped to int's range before
// it is converted and the index is clamped into the window after (floats above 2^24 round); a window with h0 < 1, w0 < 1 or
// more than slot_stride - 128 bytes is not read at all.
// This kernel keeps its own header decode, its own mode-1 copy and its own warp, the geometric kernel's stage D likewise: with
// the two warps folded into one function and this entry made an instantiation of preprocess_pixel_kernel it measured 2.5 % slower
// (122.5 against 119.5 us, profiles/loader_refactor.md) although its hot path compiled to the same instructions; the cause was not
// found, so the fold is left for a change of its own.
template <int C>
__global__ __launch_bounds__(256) void preprocess_u8_align_kernel(const unsigned char* __restrict__ slots, float* __restrict__ out, long slot_stride,
                                                                   int crop_h, int crop_w) {
#pragma clang fp contract(off)
    const int img = blockIdx.y;
    const unsigned char* slot = slots + (long)img * slot_stride;
    const int* hd = reinterpret_cast<const int*>(slot);
    const int mode = hd[0], h0 = hd[1], w0 = hd[2], y0 = hd[3], x0 = hd[4], flip = hd[5], flags = hd[6];
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= crop_h * crop_w) return;
    float* o = out + ((long)img * crop_h * crop_w + px) * C;
    if (mode == 1) {                              // finished by the worker, augmentation included
        const float* f = reinterpret_cast<const float*>(slot + ALIGN_HEADER) + (long)px * C;
        const bool fits = ((long)px + 1) * C * (long)sizeof(float) <= slot_stride - ALIGN_HEADER;      // a crop larger than the slot: zeros
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = fits ? f[c] : 0.f;
        return;
    }
    const float delta_b = __int_as_float(hd[7]), delta_h = __int_as_float(hd[8]), factor = __int_as_float(hd[9]);
    const float a0 = __int_as_float(hd[16]), a1 = __int_as_float(hd[17]), a2 = __int_as_float(hd[18]);
    const float b0 = __int_as_float(hd[19]), b1 = __int_as_float(hd[20]), b2 = __int_as_float(hd[21]);
    const bool window = h0 >= 1 && w0 >= 1 && (long)h0 * w0 <= (slot_stride - ALIGN_HEADER) / C;
    const int r = px / crop_w, cc = px - r * crop_w;
    const int col = flip ? crop_w - 1 - cc : cc;
    const float x = (float)(x0 + col), y = (float)(y0 + r);
    const float sx = (a0 * x + a1 * y) + a2, sy = (b0 * x + b1 * y) + b2;
    const float fx = floorf(sx), fy = floorf(sy), cx = fx + 1.f, cy = fy + 1.f;
    const float wl = cx - sx, wr = sx - fx, wt = cy - sy, wb = sy - fy;
    const float xmax = (float)(w0 - 1), ymax = (float)(h0 - 1);
    const bool xl = window && fx >= 0.f && fx <= xmax, xr = window && cx >= 0.f && cx <= xmax;          // false for a NaN
    const bool yt = window && fy >= 0.f && fy <= ymax, yb = window && cy >= 0.f && cy <= ymax;
    const float imax = 2147483520.f;              // the largest float an int holds: (float)(w0 - 1) is 2^31 for w0 near 2^31
    const int ixl = xl ? min((int)fminf(fx, imax), w0 - 1) : 0, ixr = xr ? min((int)fminf(cx, imax), w0 - 1) : 0;
    const int iyt = yt ? min((int)fminf(fy, imax), h0 - 1) : 0, iyb = yb ? min((int)fminf(cy, imax), h0 - 1) : 0;
    const unsigned char* img0 = slot + ALIGN_HEADER;
    const unsigned char* ptl = img0 + ((long)iyt * w0 + ixl) * C;
    const unsigned char* ptr = img0 + ((long)iyt * w0 + ixr) * C;
    const unsigned char* pbl = img0 + ((long)iyb * w0 + ixl) * C;
    const unsigned char* pbr = img0 + ((long)iyb * w0 + ixr) * C;
    const float s = (float)(1.0 / 255.0);
    const bool any = (yt || yb) && (xl || xr);
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float rtl = (yt && xl) ? (float)ptl[c] * s : 0.f, rtr = (yt && xr) ? (float)ptr[c] * s : 0.f;
        const float rbl = (yb && xl) ? (float)pbl[c] * s : 0.f, rbr = (yb && xr) ? (float)pbr[c] * s : 0.f;
        const float top = wl * rtl + wr * rtr;
        const float bot = wl * rbl + wr * rbr;
        v[c] = any ? wt * top + wb * bot : 0.f;
    }
    const float colour[3] = {delta_b, delta_h, factor};
    colour_store<C, true>(v, flags, colour, o);
}

// ------------------------------------------------------------------------------------------------
// The RESIZE transform with the geometric pair of preprocessing.py:41-71 of the reference between the crop and the flip:
// _random_zoom_in_out (resize the crop down to th x tw and back up, both TF-1.x bilinear) and _random_affine_distort (a bilinear
// warp, zero outside the image, by one of the 729 coefficient sets of `table`), as tf_face_toolbox_amd/preprocessing.py states them
// in float32.  Header: flags bit 8 = zoom, bit 16 = affine, th, tw, rnd (the table row).
//
// An output pixel reads 4 warped-source pixels, each of those 4 zoomed-down pixels, each of those 4 resized pixels, each of
// those 4 bytes: the stages are STAGED, not recomputed.  One workgroup per image; planes P (crop_h x crop_w x C floats) and Q
// (th x tw x C, at most as large) live in LDS when both fit (gray 112 x 112: 98 KB), else in the caller's workspace (the
// workgroup's own 2 planes: written and read by this workgroup only, __syncthreads() between the stages orders them):
//   A  slot bytes -> P   bilinear_tap + crop, not flipped      B  P -> Q   resize down      C  Q -> P   resize up
//   D  P -> out          warp, flip (of the OUTPUT column), colour, normalise
// An image with neither bit goes straight from the bytes to `out`, one pass, the arithmetic of the RESIZE pixel kernel.
// Words 10..12 steer addresses and are not trusted: th outside [1, crop_h] or tw outside [1, crop_w] clears the zoom, rnd outside
// [0, 728] clears the affine; every tap of B and C is clamped (bilinear_tap), the warp compares its FLOAT coordinates with the
// image's bounds before any becomes an index (a NaN or an infinity reads the zero fill).
template <int C>
__device__ __forceinline__ void resize_plane(const float* src, int sh, int sw, float* dst, int dh, int dw) {
#pragma clang fp contract(off)
    const float ry = (float)sh / (float)dh, rx = (float)sw / (float)dw;
    for (int p = threadIdx.x; p < dh * dw; p += blockDim.x) {
        const int r = p / dw;
        float v[C];
        bilinear_tap<C>(src, sh, sw, ry, rx, r, p - r * dw, v);
#pragma unroll
        for (int c = 0; c < C; ++c) dst[p * C + c] = v[c];
    }
}

constexpr int GEO_THREADS = 1024;
constexpr size_t GEO_LDS_MAX = 160 * 1024;

template <int C, bool IN_LDS>
__global__ __launch_bounds__(GEO_THREADS) void preprocess_u8_geo_kernel(const unsigned char* __restrict__ slots, float* __restrict__ out,
                                                                        long slot_stride, int in_h, int in_w, int crop_h, int crop_w,
                                                                        const float* __restrict__ table, float* ws) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float geo_planes[];
    const int img = blockIdx.x;
    const unsigned char* slot = slots + (long)img * slot_stride;
    const SlotHeader hd = read_header(slot);
    const int npx = crop_h * crop_w;
    float* o = out + (long)img * npx * C;
    if (hd.mode == 1) {
        for (int px = threadIdx.x; px < npx; px += GEO_THREADS) copy_finished<C>(slot, HEADER, slot_stride, px, o + (long)px * C);
        return;
    }
    const bool zoom = (hd.flags & 8) && hd.th >= 1 && hd.th <= crop_h && hd.tw >= 1 && hd.tw <= crop_w;
    const bool affine = (hd.flags & 16) && hd.rnd >= 0 && hd.rnd <= 728;
    const unsigned char* img0 = slot + HEADER;
    const float ry = (float)hd.h0 / (float)in_h, rx = (float)hd.w0 / (float)in_w;
    if (!zoom && !affine) {                       // one pass, bytes -> out
        for (int px = threadIdx.x; px < npx; px += GEO_THREADS) {
            const int r = px / crop_w, cc = px - r * crop_w;
            const int col = hd.flip ? crop_w - 1 - cc : cc;
            float v[C];
            bilinear_tap<C>(img0, hd.h0, hd.w0, ry, rx, hd.y0 + r, hd.x0 + col, v);
            colour_store<C, true>(v, hd.flags, hd.colour, o + (long)px * C);
        }
        return;
    }
    float* P = IN_LDS ? geo_planes : ws + (long)img * 2 * npx * C;
    float* Q = P + npx * C;
    for (int px = threadIdx.x; px < npx; px += GEO_THREADS) {                  // A
        const int r = px / crop_w;
        float v[C];
        bilinear_tap<C>(img0, hd.h0, hd.w0, ry, rx, hd.y0 + r, hd.x0 + (px - r * crop_w), v);
#pragma unroll
        for (int c = 0; c < C; ++c) P[px * C + c] = v[c];
    }
    __syncthreads();
    if (zoom) {                                   // uniform over the workgroup: the header decides
        resize_plane<C>(P, crop_h, crop_w, Q, hd.th, hd.tw);                   // B
        __syncthreads();
        resize_plane<C>(Q, hd.th, hd.tw, P, crop_h, crop_w);                   // C
        __syncthreads();
    }
    float a0 = 1.f, a1 = 0.f, a2 = 0.f, b0 = 0.f, b1 = 1.f, b2 = 0.f;
    if (affine) {
        const float* t = table + hd.rnd * 6;
        a0 = t[0]; a1 = t[1]; a2 = t[2]; b0 = t[3]; b1 = t[4]; b2 = t[5];
    }
    const float xmax = (float)(crop_w - 1), ymax = (float)(crop_h - 1);
    for (int px = threadIdx.x; px < npx; px += GEO_THREADS) {                  // D
        const int r = px / crop_w, cc = px - r * crop_w;
        const int col = hd.flip ? crop_w - 1 - cc : cc;
        float v[C];
        if (affine) {
            const float x = (float)col, y = (float)r;
            const float sx = (a0 * x + a1 * y) + a2, sy = (b0 * x + b1 * y) + b2;
            const float fx = floorf(sx), fy = floorf(sy), cx = fx + 1.f, cy = fy + 1.f;
            const float wl = cx - sx, wr = sx - fx, wt = cy - sy, wb = sy - fy;
            const bool xl = fx >= 0.f && fx <= xmax, xr = cx >= 0.f && cx <= xmax;          // false for a NaN
            const bool yt = fy >= 0.f && fy <= ymax, yb = cy >= 0.f && cy <= ymax;
            const int ixl = xl ? (int)fx : 0, ixr = xr ? (int)cx : 0, iyt = yt ? (int)fy : 0, iyb = yb ? (int)cy : 0;
            const float* ptl = P + (iyt * crop_w + ixl) * C;
            const float* ptr = P + (iyt * crop_w + ixr) * C;
            const float* pbl = P + (iyb * crop_w + ixl) * C;
            const float* pbr = P + (iyb * crop_w + ixr) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float rtl = (yt && xl) ? ptl[c] : 0.f, rtr = (yt && xr) ? ptr[c] : 0.f;
                const float rbl = (yb && xl) ? pbl[c] : 0.f, rbr = (yb && xr) ? pbr[c] : 0.f;
                const float top = wl * rtl + wr * rtr;
                const float bot = wl * rbl + wr * rbr;
                v[c] = wt * top + wb * bot;
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = P[(r * crop_w + col) * C + c];
        }
        colour_store<C, true>(v, hd.flags, hd.colour, o + (long)px * C);
    }
}

// ------------------------------------------------------------------------------------------------
// Raw slots from a pre-decoded image pack resident in device memory (fte.h: fte_pack_gather_slots): slot i = the 64 header bytes
// the worker wrote for image i, then row clamp(index[i]) of the pack.  A copy in 16-byte chunks -- rows, headers and slots are
// 16-byte aligned and every stride is a multiple of 64 --; blockIdx.y strides over the images, blockIdx.x * 256 + threadIdx.x
// over a slot's chunks, so no index is ever divided.  The index is device data: it is clamped before it forms an address.
// Every byte offset is 64-bit (row * row_stride passes 2^32 for real packs).  No LDS, no atomics: a slot byte has one writer.
__global__ void __launch_bounds__(256) pack_gather_slots_kernel(const uint4* __restrict__ rows, long num_rows, long row_chunks,
                                                                const int64_t* __restrict__ index, const uint4* __restrict__ headers,
                                                                uint4* __restrict__ slots, int n, long slot_chunks) {
    const long chunks = 4 + row_chunks;                             // of one slot's written part: 64 header bytes + the row
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        long r = index[i];
        r = r < 0 ? 0 : r >= num_rows ? num_rows - 1 : r;
        const uint4* src = rows + (long)r * row_chunks;
        const uint4* hd = headers + (long)i * 4;
        uint4* dst = slots + (long)i * slot_chunks;
        for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (long)gridDim.x * 256)
            dst[c] = c < 4 ? hd[c] : src[c - 4];
    }
}

}  // namespace

hipError_t k_preprocess_u8(const unsigned char* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w,
                           int crop_h, int crop_w, hipStream_t st) {
    return launch_pixel(preprocess_pixel_kernel<3, false>, preprocess_pixel_kernel<1, false>, n, channels, crop_h, crop_w, st,
                        slots, out, slot_stride, in_h, in_w, crop_h, crop_w);
}

hipError_t k_preprocess_u8_aug(const unsigned char* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w,
                               int crop_h, int crop_w, hipStream_t st) {
    return launch_pixel(preprocess_pixel_kernel<3, true>, preprocess_pixel_kernel<1, true>, n, channels, crop_h, crop_w, st,
                        slots, out, slot_stride, in_h, in_w, crop_h, crop_w);
}

hipError_t k_preprocess_u8_align(const unsigned char* slots, float* out, int n, long slot_stride, int channels, int crop_h, int crop_w,
                                 hipStream_t st) {
    return launch_pixel(preprocess_u8_align_kernel<3>, preprocess_u8_align_kernel<1>, n, channels, crop_h, crop_w, st,
                        slots, out, slot_stride, crop_h, crop_w);
}

size_t k_preprocess_u8_geo_ws_bytes(int n, int channels, int crop_h, int crop_w) {
    const size_t planes = (size_t)2 * crop_h * crop_w * channels * sizeof(float);
    return planes <= GEO_LDS_MAX ? 0 : planes * n;
}

hipError_t k_preprocess_u8_geo(const unsigned char* slots, float* out, int n, long slot_stride, int channels, int in_h, int in_w,
                               int crop_h, int crop_w, const float* table, void* ws, hipStream_t st) {
    const size_t planes = (size_t)2 * crop_h * crop_w * channels * sizeof(float);
    const bool in_lds = planes <= GEO_LDS_MAX;
    const size_t lds = in_lds ? planes : 0;
#define FTE_GEO(C_, L_) do { \
        auto kern = preprocess_u8_geo_kernel<C_, L_>; \
        if (lds > 48 * 1024) { \
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
            if (e != hipSuccess) return e; \
        } \
        kern<<<dim3(n), GEO_THREADS, lds, st>>>(slots, out, slot_stride, in_h, in_w, crop_h, crop_w, table, (float*)ws); } while (0)
    if (channels == 3) { if (in_lds) FTE_GEO(3, true); else FTE_GEO(3, false); }
    else { if (in_lds) FTE_GEO(1, true); else FTE_GEO(1, false); }
#undef FTE_GEO
    return hipGetLastError();
}

hipError_t k_pack_gather_slots(const unsigned char* rows, long num_rows, long row_stride, const int64_t* index,
                               const unsigned char* headers, unsigned char* slots, int n, long slot_stride, int cus, hipStream_t st) {
    // memory-bound: at most ~8 blocks of 256 threads per CU, the loops stride over the rest
    const long cap = 8L * (cus > 0 ? cus : 256);
    const long per_slot = ((64 + row_stride) / 16 + 255) / 256;
    const long gx = per_slot < cap ? per_slot : cap;
    long gy = cap / gx < 1 ? 1 : cap / gx;
    if (gy > n) gy = n;
    if (gy > 65535) gy = 65535;
    pack_gather_slots_kernel<<<dim3((unsigned)gx, (unsigned)gy), 256, 0, st>>>((const uint4*)rows, num_rows, row_stride / 16, index,
                                                                             (const uint4*)headers, (uint4*)slots, n, slot_stride / 16);
    return hipGetLastError();
}
