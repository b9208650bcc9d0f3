// Accuracy of __expf (what the sigmoids of csrc/gate.hip and csrc/cpam.hip call) against fp64 exp on gfx950, per range of |x|.
// hipcc --offload-arch=gfx950 -O3 tools/micro/expf_error.hip -o tools/micro/expf_error && tools/micro/expf_error
// Prints, for each bin lo <= |x| < hi and both signs, the worst |__expf(x) - exp(x)| / exp(x) in units of 2^-24 over 2^24 evenly spaced
// arguments.  The figures go into tests/ref64.py (EXPF_ULPS) with the margin stated there; profiles/r08_gates_ref64.txt keeps the output of the run they come from.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

constexpr int THREADS = 256, BLOCKS = 1024, PER = 64;   // 2^24 samples per (bin, sign)

__global__ void expf_err_kernel(float lo, float hi, float sign, double* worst, float* at) {
  const int tid = blockIdx.x * THREADS + threadIdx.x;
  const long long n = (long long)THREADS * BLOCKS * PER;
  double w = 0.0;
  float wx = 0.f;
  for (int i = 0; i < PER; ++i) {
    const long long k = (long long)i * THREADS * BLOCKS + tid;
    const float x = sign * (lo + (hi - lo) * (float)((double)k / (double)n));
    const double ref = exp((double)x);
    const double err = fabs((double)__expf(x) - ref) / ref;
    if (err > w) { w = err; wx = x; }
  }
  worst[tid] = w;
  at[tid] = wx;
}

int main() {
  const int n = THREADS * BLOCKS;
  double* d_w;
  float* d_x;
  if (hipMalloc(&d_w, n * sizeof(double)) != hipSuccess || hipMalloc(&d_x, n * sizeof(float)) != hipSuccess) { printf("hipMalloc failed\n"); return 1; }
  std::vector<double> w(n);
  std::vector<float> x(n);
  const float edges[] = {0.f, 1.f, 2.f, 4.f, 8.f, 16.f, 32.f, 64.f};
  printf("__expf vs fp64 exp, worst relative error in units of 2^-24, %d arguments per line\n", n * PER);
  for (int b = 0; b + 1 < (int)(sizeof(edges) / sizeof(edges[0])); ++b)
    for (float sign : {1.f, -1.f}) {
      hipLaunchKernelGGL(expf_err_kernel, dim3(BLOCKS), dim3(THREADS), 0, 0, edges[b], edges[b + 1], sign, d_w, d_x);
      if (hipMemcpy(w.data(), d_w, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(x.data(), d_x, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { printf("hipMemcpy failed\n"); return 1; }
      int at = 0;
      for (int i = 1; i < n; ++i) if (w[i] > w[at]) at = i;
      printf("  %c[%2g, %2g)  worst %8.3f x 2^-24  at x = %.9g\n", sign > 0 ? '+' : '-', edges[b], edges[b + 1], w[at] * 16777216.0, x[at]);
    }
  (void)hipFree(d_w); (void)hipFree(d_x);
  return 0;
}
