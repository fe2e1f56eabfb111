// Dependent-issue latency of the fp64 instructions on the small-batch solve's chain, for ONE wavefront alone on its
// SIMD: cycles per instruction at ILP 1 (every instruction reads the result of the one in front) against ILP 8
// (eight independent chains, the issue rate).  latency in issue slots = ILP 1 figure / ILP 8 figure.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/dep_latency_micro.hip -o tools/micro/dep_latency_micro
// Cases: v_fma_f64 on v_fma_f64; v_mul_f64 on v_mul_f64; v_rcp_f64 followed by its Newton v_fma_f64 (the pair, as in
// rcp64 of msnap_sweep.h: the fma reads the reciprocal, the next reciprocal reads the fma).
#include <hip/hip_runtime.h>
#include <cstdio>

enum Case { FMA = 0, MUL = 1, RCP_FMA = 2 };

template <int CASE, int ILP>
__global__ void __launch_bounds__(64) chain(double *out, int iters, long long *cycles) {
  double a[ILP];
#pragma unroll
  for (int k = 0; k < ILP; ++k) a[k] = 1.0 + threadIdx.x * 1e-3 + k;
  const double m = 1.0000001, c = 0.5;
  long long t0 = __builtin_amdgcn_s_memtime();
  for (int i = 0; i < iters; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
      for (int k = 0; k < ILP; ++k) {
        if (CASE == FMA) a[k] = __builtin_fma(a[k], m, c);
        if (CASE == MUL) a[k] = a[k] * m;
        if (CASE == RCP_FMA) a[k] = __builtin_fma(-a[k], __builtin_amdgcn_rcp(a[k]), 2.0);   // stays near 1
      }
  }
  long long t1 = __builtin_amdgcn_s_memtime();
  double s = 0;
#pragma unroll
  for (int k = 0; k < ILP; ++k) s += a[k];
  out[threadIdx.x] = s;
  if (threadIdx.x == 0) cycles[0] = t1 - t0;
}

template <int CASE, int ILP>
double run(double *out, long long *cyc) {
  const int iters = 2000;
  for (int rep = 0; rep < 2; ++rep) {     // the second launch is the measurement (code and clocks warm)
    hipLaunchKernelGGL((chain<CASE, ILP>), dim3(1), dim3(64), 0, 0, out, iters, cyc);
    hipDeviceSynchronize();
  }
  long long h = 0;
  hipMemcpy(&h, cyc, 8, hipMemcpyDeviceToHost);
  const int per_step = CASE == RCP_FMA ? 2 : 1;     // instructions per chain step
  return (double)h / (iters * 16.0 * ILP * per_step);
}

template <int CASE>
void report(const char *name, double *out, long long *cyc) {
  const double d1 = run<CASE, 1>(out, cyc), d8 = run<CASE, 8>(out, cyc);
  printf("%-28s ILP 1: %6.2f  ILP 8: %6.2f s_memtime ticks per instruction -> latency %.2f issue slots\n", name, d1, d8,
         d1 / d8);
}

int main() {
  double *out;
  long long *cyc;
  if (hipMalloc(&out, 64 * sizeof(double)) != hipSuccess || hipMalloc(&cyc, sizeof(long long)) != hipSuccess) {
    printf("no device memory\n");
    return 1;
  }
  report<FMA>("v_fma_f64 -> v_fma_f64", out, cyc);
  report<MUL>("v_mul_f64 -> v_mul_f64", out, cyc);
  report<RCP_FMA>("v_rcp_f64 -> v_fma_f64 (pair)", out, cyc);
  hipFree(out);
  hipFree(cyc);
  return 0;
}
