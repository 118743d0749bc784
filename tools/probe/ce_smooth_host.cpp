// The smoothed cross-entropy kernels (csrc/train_kernels.hip, between the "[ce_smooth: begin]" / "[ce_smooth: end]" markers)
// run on the HOST: one thread per lane, 64 per wave, wave shuffles through a barrier.  Built with AddressSanitizer it checks
// what a device run cannot show safely: no access outside the buffers for any V, row base alignment and mode; every loss and
// gradient element written; ignored rows exactly 0; values against a double-precision evaluation of the formulas.  No GPU.
// threadIdx / blockIdx, float4, __shfl_xor, wsum and wmax below are HOST stand-ins written for this program, not the device
// ones: they must be kept in step with csrc/train_common.h by hand (same xor-butterfly order, so the sums round alike).
//   cd tools/probe && sed -n '/\[ce_smooth: begin\]/,/\[ce_smooth: end\]/p' ../../doc2tex_amd/csrc/train_kernels.hip > ce_smooth.inc
//   g++ -std=c++20 -O1 -g -fsanitize=address,undefined -fno-sanitize=alignment -pthread ce_smooth_host.cpp -o ce_smooth_host
//   ./ce_smooth_host        (lines only for cases beyond 1e-6 of the tensor's maximum: expected for V <= 3 alone)
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
struct D3 { int x, y, z; };
thread_local D3 threadIdx, blockIdx;
using std::min;
struct float4 { float x, y, z, w; };
inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
static std::barrier<> bar(64);
static float slots[64];
inline float __shfl_xor(float v, int o, int) {
  int lane = threadIdx.x & 63;
  slots[lane] = v;
  bar.arrive_and_wait();
  float r = slots[lane ^ o];
  bar.arrive_and_wait();
  return r;
}
inline float wsum(float v) { for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64); return v; }
inline float wmax(float v) { for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64)); return v; }
namespace d2t {
#include "ce_smooth.inc"
}
template <class F> void launch(int rows, F f) {
  for (int b = 0; b < (rows + 3) / 4; ++b)
    for (int w = 0; w < 4; ++w) {
      std::vector<std::thread> th;
      for (int l = 0; l < 64; ++l) th.emplace_back([=] { threadIdx = {w * 64 + l, 0, 0}; blockIdx = {b, 0, 0}; f(); bar.arrive_and_wait(); });
      for (auto& t : th) t.join();
    }
}
int main() {
  int shapes[][2] = {{4, 11}, {5, 1025}, {37, 93}, {6, 500}, {3, 1}, {5, 2}, {5, 3}, {4, 64}, {5, 65}, {6, 67}, {5, 16384}, {3, 16381}};
  double worst_l = 0, worst_g = 0;
  srand(1);
  for (auto& sh : shapes) for (int mode = 0; mode < 2; ++mode) for (int useW = 0; useW < (mode ? 1 : 2); ++useW) for (int xo = 0; xo < 4; ++xo) for (int dxo : {xo, (xo + 2) & 3}) {
    int rows = sh[0], V = sh[1];
    size_t n = (size_t)rows * V;
    // exact-size heap blocks so that ASan sees any access one element past the end; malloc blocks are 16-byte aligned, so
    // xa + xo / da + dxo give every (mis)alignment of the two bases
    float* xa = (float*)malloc((n + xo) * 4); float* x = xa + xo;
    float* da = (float*)malloc((n + dxo) * 4); float* dx = da + dxo;
    float* w = useW ? (float*)malloc(V * 4) : nullptr;
    int64_t* t = (int64_t*)malloc(rows * 8);
    float *loss = (float*)malloc(rows * 4), *lse = (float*)malloc(rows * 4), *mass = (float*)malloc(rows * 4), *g = (float*)malloc(rows * 4);
    for (size_t i = 0; i < n; ++i) { x[i] = 3.f * ((rand() / (float)RAND_MAX) * 2 - 1) * 2; dx[i] = NAN; }
    if (V > 4) x[5 % V] = -INFINITY;  // a masked logit
    for (int v = 0; v < V; ++v) if (w) w[v] = 0.5f + rand() / (float)RAND_MAX;
    long long pad = V > 2 ? 2 : 0, ignore = mode ? pad : 0;
    for (int r = 0; r < rows; ++r) { t[r] = rand() % V; g[r] = 0.5f + rand() / (float)RAND_MAX; loss[r] = NAN; }
    if (rows > 1) t[1] = ignore;
    if (rows > 2) t[2] = V + 5;
    float on = 0.9f, off = mode ? (V > 2 ? 0.1f / (V - 2 > 0 ? V - 2 : 1) : 0.05f) : 0.1f / V;
    if (V > 4 && !mode) off = (xo & 1) ? off : 0.f;  // smoothing 0 with a -inf logit must stay finite
    if (V > 4 && !mode && off != 0.f) x[5 % V] = -3.f;
    launch(rows, [=] { d2t::ce_smooth_fwd_kernel(x, t, w, loss, lse, mass, rows, V, ignore, on, off, mode, pad); });
    launch(rows, [=] { d2t::ce_smooth_bwd_kernel(x, t, w, lse, mass, g, dx, rows, V, ignore, on, off, mode, pad); });
    double ml = 0, mg = 0, el = 0, eg = 0;
    for (int r = 0; r < rows; ++r) {
      bool live = !(t[r] == ignore || t[r] < 0 || t[r] >= V);
      const float* xr = x + (size_t)r * V;
      double mx = -INFINITY; for (int v = 0; v < V; ++v) mx = std::max(mx, (double)xr[v]);
      double s = 0; for (int v = 0; v < V; ++v) s += exp(xr[v] - mx);
      double l = mx + log(s), L = 0, M = 0;
      std::vector<double> mv(V, 0.0);
      if (live) for (int v = 0; v < V; ++v) {
        double wv = w ? w[v] : 1.0;
        bool inS = mode ? (v != t[r] && v != pad) : true;
        mv[v] = (v == t[r] ? (double)on * (w ? w[t[r]] : 1.0) : 0.0) + (inS ? (double)off * wv : 0.0);
        M += mv[v]; if (mv[v] != 0) L += mv[v] * (l - xr[v]);
      }
      if (std::isnan(loss[r])) { printf("loss row %d not written\n", r); return 1; }
      if (!live && loss[r] != 0.f) { printf("ignored row %d loss %g\n", r, loss[r]); return 1; }
      el = std::max(el, fabs(loss[r] - L)); ml = std::max(ml, fabs(L));
      for (int v = 0; v < V; ++v) {
        double d = live ? g[r] * (M * exp(xr[v] - l) - mv[v]) : 0.0;
        float got = dx[(size_t)r * V + v];
        if (std::isnan(got)) { printf("dx[%d][%d] not written (V %d mode %d xo %d dxo %d)\n", r, v, V, mode, xo, dxo); return 1; }
        if (!live && got != 0.f) { printf("ignored row grad\n"); return 1; }
        eg = std::max(eg, fabs(got - d)); mg = std::max(mg, fabs(d));
      }
    }
    double rl = ml > 0 ? el / ml : el, rg = mg > 0 ? eg / mg : eg;
    if (rl > 1e-6 || rg > 1e-6) printf("rows %d V %d mode %d w %d xo %d dxo %d: loss %.2e grad %.2e\n", rows, V, mode, useW, xo, dxo, rl, rg);
    worst_l = std::max(worst_l, rl); worst_g = std::max(worst_g, rg);
    free(xa); free(da); free(w); free(t); free(loss); free(lse); free(mass); free(g);
  }
  printf("worst loss %.2e grad %.2e\n", worst_l, worst_g);
  return 0;
}
