// Patch-wise evaluation (`split_input_params`, ddpm.py:565-652,904-986): crops as batch items.
//   ldmk_patch_unfold  (n,c,h,w) -> (ly*lx*n, c, kh, kw), patch-major like torch.nn.Unfold's L axis: a pure copy
//   ldmk_patch_fold    the weighted overlap-add of the crops' outputs divided by the accumulated weight, in GATHER form:
//                      one output element per lane-slot sums the (at most ceil(kh/sh) * ceil(kw/sw)) crops that cover it in
//                      ascending patch index -- no atomics, one fixed order, bit-reproducible
// Both are HBM-bound copies: 16-byte accesses along w when w, kw, sw and the bases are multiples of 4 floats (then the four
// pixels of a group lie in the same crops at consecutive, aligned columns), a scalar kernel otherwise; the host chooses.
#include "ldmk_common.h"

namespace {

static inline unsigned grid_for(long long total, int block = 256, int cap = 4096) {
  long long g = (total + block - 1) / block;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (unsigned)g;
}

struct PatchGeom {
  int n, c, h, w, kh, kw, sh, sw, ly, lx;
};

// V = floats per lane-slot along w (1 or 4)
template <int V>
__global__ __launch_bounds__(256) void patch_unfold_kernel(const float* __restrict__ x, float* __restrict__ patches, PatchGeom g,
                                                           long long total) {
  const int kwv = g.kw / V;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    long long r = i;
    const int px = (int)(r % kwv) * V;  r /= kwv;
    const int py = (int)(r % g.kh);     r /= g.kh;
    const int ch = (int)(r % g.c);      r /= g.c;
    const int b = (int)(r % g.n);       r /= g.n;
    const int l = (int)r;
    const int iy = l / g.lx, ix = l - iy * g.lx;
    const long long src = (((long long)b * g.c + ch) * g.h + (iy * g.sh + py)) * g.w + (ix * g.sw + px);
    if constexpr (V == 4)
      *reinterpret_cast<float4*>(patches + i * 4) = *reinterpret_cast<const float4*>(x + src);
    else
      patches[i] = x[src];
  }
}

template <int V>
__global__ __launch_bounds__(256) void patch_fold_kernel(const float* __restrict__ patches, const float* __restrict__ weight,
                                                         const float* __restrict__ norm, float* __restrict__ out, PatchGeom g,
                                                         long long total) {
  const int wv = g.w / V;
  const int L = g.ly * g.lx;
  const long long crop = (long long)g.kh * g.kw;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    long long r = i;
    const int x = (int)(r % wv) * V;  r /= wv;
    const int y = (int)(r % g.h);     r /= g.h;
    const int ch = (int)(r % g.c);    r /= g.c;
    const int b = (int)r;
    // crops iy with iy*sh <= y < iy*sh + kh (likewise ix); V == 4: x, sw, kw are multiples of 4, so x .. x+3 share them
    const int iy0 = y < g.kh ? 0 : (y - g.kh) / g.sh + 1;
    const int iy1 = min(g.ly - 1, y / g.sh);
    const int ix0 = x < g.kw ? 0 : (x - g.kw) / g.sw + 1;
    const int ix1 = min(g.lx - 1, x / g.sw);
    float acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f;
    for (int iy = iy0; iy <= iy1; ++iy) {
      const int py = y - iy * g.sh;
      for (int ix = ix0; ix <= ix1; ++ix) {
        const int px = x - ix * g.sw;
        const int l = iy * g.lx + ix;
        const long long src = (((long long)l * g.n + b) * g.c + ch) * crop + (long long)py * g.kw + px;
        const float* wp = weight + ((long long)py * g.kw + px) * L + l;
        float p[V];
        if constexpr (V == 4) {
          const float4 q = *reinterpret_cast<const float4*>(patches + src);
          p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w;
        } else {
          p[0] = patches[src];
        }
        // the reference rounds the product (o * weighting) before Fold adds it: no contraction into an fma
#pragma unroll
        for (int v = 0; v < V; ++v) acc[v] = __fadd_rn(acc[v], __fmul_rn(p[v], wp[(long long)v * L]));
      }
    }
    const long long dst = (((long long)b * g.c + ch) * g.h + y) * g.w + x;
    if constexpr (V == 4) {
      const float4 nv = *reinterpret_cast<const float4*>(norm + (long long)y * g.w + x);
      float4 o;
      o.x = __fdiv_rn(acc[0], nv.x); o.y = __fdiv_rn(acc[1], nv.y);
      o.z = __fdiv_rn(acc[2], nv.z); o.w = __fdiv_rn(acc[3], nv.w);
      *reinterpret_cast<float4*>(out + dst) = o;
    } else {
      out[dst] = __fdiv_rn(acc[0], norm[(long long)y * g.w + x]);      // a real division, as the reference's `/ normalization`
    }
  }
}

static int check_geometry(const char* who, int n, int c, int h, int w, int kh, int kw, int sh, int sw, int ly, int lx) {
  LDMK_REQUIRE(n > 0 && c > 0 && h > 0 && w > 0 && kh > 0 && kw > 0 && sh > 0 && sw > 0 && ly > 0 && lx > 0,
               "%s: sizes must be positive (n=%d c=%d h=%d w=%d kh=%d kw=%d sh=%d sw=%d ly=%d lx=%d)", who, n, c, h, w, kh, kw, sh,
               sw, ly, lx);
  LDMK_REQUIRE(kh <= h && kw <= w, "%s: patch %dx%d larger than the image %dx%d", who, kh, kw, h, w);
  LDMK_REQUIRE(ly == (h - kh) / sh + 1 && lx == (w - kw) / sw + 1, "%s: ly=%d lx=%d, but %dx%d patches at stride %dx%d give %dx%d on "
               "a %dx%d image", who, ly, lx, kh, kw, sh, sw, (h - kh) / sh + 1, (w - kw) / sw + 1, h, w);
  LDMK_REQUIRE((ly - 1) * sh + kh == h && (lx - 1) * sw + kw == w, "%s: %dx%d patches at stride %dx%d do not cover a %dx%d image "
               "(the last patch ends at row %d, column %d): uncovered pixels would be 0/0", who, kh, kw, sh, sw, h, w,
               (ly - 1) * sh + kh, (lx - 1) * sw + kw);
  LDMK_REQUIRE((long long)ly * lx * n < (1LL << 31), "%s: too many patches", who);
  return LDMK_OK;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int ldmk_patch_unfold(const float* x, float* patches, int n, int c, int h, int w, int kh, int kw, int sh, int sw, int ly,
                                 int lx, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(x && patches, "ldmk_patch_unfold: null pointer");
  if (int rc = check_geometry("ldmk_patch_unfold", n, c, h, w, kh, kw, sh, sw, ly, lx)) return rc;
  const PatchGeom g = {n, c, h, w, kh, kw, sh, sw, ly, lx};
  const long long total = (long long)ly * lx * n * c * kh * kw;
  const bool vec = w % 4 == 0 && kw % 4 == 0 && sw % 4 == 0 && aligned16(x) && aligned16(patches);
  if (vec)
    hipLaunchKernelGGL(patch_unfold_kernel<4>, dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream, x, patches, g, total / 4);
  else
    hipLaunchKernelGGL(patch_unfold_kernel<1>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, patches, g, total);
  return ldmk::check_launch("ldmk_patch_unfold");
}

extern "C" int ldmk_patch_fold(const float* patches, const float* weight, const float* norm, float* out, int n, int c, int h, int w,
                               int kh, int kw, int sh, int sw, int ly, int lx, void* stream) {
  LDMK_ENTER();
  LDMK_REQUIRE(patches && weight && norm && out, "ldmk_patch_fold: null pointer");
  if (int rc = check_geometry("ldmk_patch_fold", n, c, h, w, kh, kw, sh, sw, ly, lx)) return rc;
  const PatchGeom g = {n, c, h, w, kh, kw, sh, sw, ly, lx};
  const long long total = (long long)n * c * h * w;
  const bool vec = w % 4 == 0 && kw % 4 == 0 && sw % 4 == 0 && aligned16(patches) && aligned16(norm) && aligned16(out);
  if (vec)
    hipLaunchKernelGGL(patch_fold_kernel<4>, dim3(grid_for(total / 4)), dim3(256), 0, (hipStream_t)stream, patches, weight, norm, out,
                       g, total / 4);
  else
    hipLaunchKernelGGL(patch_fold_kernel<1>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, patches, weight, norm, out, g,
                       total);
  return ldmk::check_launch("ldmk_patch_fold");
}
