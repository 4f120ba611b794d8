// explain_kernel (kernels_explain.cuh) for the tables with the Fq12 gadget, a unit of their own for the compile time.
#include "prover_ctx.hpp"
#include "kernels_explain.cuh"

void launch_explain_kernel_fq12(int kind, dim3 grid, hipStream_t st, const ExplainParams& ep, const u64* apow0, const u64* apow1, const void* pic) {
  if (kind == SBN_AIR_FQ12_EXP) hipLaunchKernelGGL(explain_kernel<4>, grid, dim3(256), 0, st, ep, apow0, apow1, pic);
  else if (kind == SBN_AIR_FQ12_EXP_U64) hipLaunchKernelGGL(explain_kernel<6>, grid, dim3(256), 0, st, ep, apow0, apow1, pic);
  else hipLaunchKernelGGL(explain_kernel<8>, grid, dim3(256), 0, st, ep, apow0, apow1, pic);
}
