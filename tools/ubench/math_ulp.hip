// Largest error of the device's expf and logf, in ulps against the host's double exp / log, over the arguments that
// soft_aggregate (rmnet_amd/csrc/epilogue.hip) produces: expf on [-34, 0] (z - max, logit - max) and on -200, logf on
// [1e-8, 1e8] (em / (1 - em) with em in [1e-7, 1 - 1e-7]).  Also whether expf(0) == 1 and logf(1) == 0 exactly.
// tests/glue_ref.py takes E_MEASURED / L_MEASURED from this program's output (profiles/r14_a_glue_tests.md).
// For the exact-fp32 memory read (mr_main / mr_combine, rmnet_amd/csrc/memory_read.hip), whose deferred soft-max reference takes
// expf at arguments up to +30 and far below -34: expf on [-64, 32], and the fast __expf of its rescale factor alpha on [-160, -30]
// (relative error where the result is a normal number, absolute error below).  tests/exact_read_ref.py takes E_MEASURED_WIDE and
// A_MEASURED from these lines (profiles/r31_a_exact_read_tests.md).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/math_ulp.hip -o tools/ubench/math_ulp && tools/ubench/math_ulp
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)
__global__ void k(const float* in, float* e, float* l, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) { e[i] = expf(in[i]); l[i] = logf(in[n + i]); }
}
__global__ void k_wide(const float* in, float* e, float* f, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) { e[i] = expf(in[i]); f[i] = __expf(in[n + i]); }
}
static double ulps(float got, double ref) {
  int ex;
  frexp(ref, &ex);                                   // |ref| in [2^(ex-1), 2^ex): one ulp of fp32 there is 2^(ex - 24)
  return fabs((double)got - ref) / ldexp(1.0, ex - 24);
}
int main() {
  const int n = 1 << 22;
  std::vector<float> in(2 * n), e(n), l(n);
  for (int i = 0; i < n; ++i) {
    in[i] = (float)(-34.0 * (double)i / (n - 1));                              // expf: dense on [-34, 0]
    in[n + i] = (float)exp(log(1e-8) + (log(1e8) - log(1e-8)) * (double)i / (n - 1));   // logf: geometric on [1e-8, 1e8]
  }
  in[0] = 0.0f;
  in[1] = -200.0f;
  in[n + 1] = 1.0f;
  float *din, *de, *dl;
  CK(hipMalloc(&din, 2 * n * sizeof(float)));
  CK(hipMalloc(&de, n * sizeof(float)));
  CK(hipMalloc(&dl, n * sizeof(float)));
  CK(hipMemcpy(din, in.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k, dim3(n / 256), dim3(256), 0, 0, din, de, dl, n);
  CK(hipGetLastError());
  CK(hipMemcpy(e.data(), de, n * sizeof(float), hipMemcpyDeviceToHost));
  CK(hipMemcpy(l.data(), dl, n * sizeof(float), hipMemcpyDeviceToHost));
  double me = 0, ml = 0, ml1 = 0;
  float ae = 0, al = 0;
  for (int i = 0; i < n; ++i) {
    if (i == 1) continue;                                                      // (-200 and 1 are reported on their own)
    const double ue = ulps(e[i], exp((double)in[i]));
    if (ue > me) { me = ue; ae = in[i]; }
    const double rl = log((double)in[n + i]);
    const double ul = ulps(l[i], rl);
    if (ul > ml) { ml = ul; al = in[n + i]; }
    if (fabs(rl) < 1.0 && ul > ml1) ml1 = ul;                                  // (near 1, where the result is small)
  }
  printf("MATH expf: max %.3f ulp at %.9g over %d points of [-34, 0]\n", me, ae, n);
  printf("MATH logf: max %.3f ulp at %.9g over %d points of [1e-8, 1e8] (|log| < 1: max %.3f ulp)\n", ml, al, n, ml1);
  printf("MATH expf(0) = %.9g (%s), expf(-200) = %.9g, logf(1) = %.9g (%s)\n", e[0], e[0] == 1.0f ? "exact" : "NOT exact", e[1],
         l[1], l[1] == 0.0f ? "exact" : "NOT exact");
  // ---- the exact-fp32 memory read's arguments: expf on [-64, 32], __expf on [-160, -30]
  for (int i = 0; i < n; ++i) {
    in[i] = (float)(-64.0 + 96.0 * (double)i / (n - 1));
    in[n + i] = (float)(-160.0 + 130.0 * (double)i / (n - 1));
  }
  CK(hipMemcpy(din, in.data(), 2 * n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_wide, dim3(n / 256), dim3(256), 0, 0, din, de, dl, n);
  CK(hipGetLastError());
  CK(hipMemcpy(e.data(), de, n * sizeof(float), hipMemcpyDeviceToHost));
  CK(hipMemcpy(l.data(), dl, n * sizeof(float), hipMemcpyDeviceToHost));
  double mw = 0, mpos = 0, mrel = 0, mabs = 0;
  float aw = 0, arel = 0, aabs = 0;
  for (int i = 0; i < n; ++i) {
    const double ue = ulps(e[i], exp((double)in[i]));
    if (ue > mw) { mw = ue; aw = in[i]; }
    if (in[i] > 0.0f && ue > mpos) mpos = ue;
    const double rf = exp((double)in[n + i]);
    if (rf >= ldexp(1.0, -126)) {
      const double rel = fabs((double)l[i] - rf) / rf;
      if (rel > mrel) { mrel = rel; arel = in[n + i]; }
    } else {
      const double ab = fabs((double)l[i] - rf);
      if (ab > mabs) { mabs = ab; aabs = in[n + i]; }
    }
  }
  printf("MATH expf wide: max %.3f ulp at %.9g over %d points of [-64, 32] (arguments > 0: max %.3f ulp)\n", mw, aw, n, mpos);
  printf("MATH __expf: max relative error %.3e (%.2f x 2^-23) at %.9g over %d points of [-160, -30] with a normal result; "
         "below: max absolute error %.3e at %.9g\n", mrel, mrel * 8388608.0, arel, n, mabs, aabs);
  (void)hipFree(din); (void)hipFree(de); (void)hipFree(dl);
  return 0;
}
