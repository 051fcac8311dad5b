// Row gather of the minibatch prelude: dst_k[e] = src_k[ids[e]] for up to DGPPO_GATHER_MAX tensors that share one id list,
// in ONE launch (the update gathers 6-7 per-env tensors by the minibatch's env ids).  Pure data movement.
#include "common.h"

struct GatherArgs {
  const char* src[DGPPO_GATHER_MAX];
  char* dst[DGPPO_GATHER_MAX];
  long row_bytes[DGPPO_GATHER_MAX], src_stride[DGPPO_GATHER_MAX];
  int vec[DGPPO_GATHER_MAX];          // 1: 16-byte units, 0: dwords
  const int32_t* ids;
  int n_ids;
};

// blockIdx.z = descriptor, blockIdx.y strides over the ids, blockIdx.x over the units of a row
__global__ void __launch_bounds__(256) gather_rows_kernel(GatherArgs a) {
  const int k = blockIdx.z;
  const long units = a.vec[k] ? a.row_bytes[k] >> 4 : a.row_bytes[k] >> 2;
  const long u0 = (long)blockIdx.x * blockDim.x + threadIdx.x, du = (long)gridDim.x * blockDim.x;
  if (u0 >= units) return;
  for (int e = blockIdx.y; e < a.n_ids; e += gridDim.y) {
    const char* s = a.src[k] + (size_t)a.ids[e] * a.src_stride[k];
    char* d = a.dst[k] + (size_t)e * a.row_bytes[k];
    if (a.vec[k]) {
      for (long u = u0; u < units; u += du) reinterpret_cast<uint4*>(d)[u] = reinterpret_cast<const uint4*>(s)[u];
    } else {
      for (long u = u0; u < units; u += du) reinterpret_cast<uint32_t*>(d)[u] = reinterpret_cast<const uint32_t*>(s)[u];
    }
  }
}

extern "C" int32_t dgppo_gather_rows(const dgppo_gather_desc* descs, int32_t n_desc, const int32_t* ids, int32_t n_ids,
                                     void* stream) {
  DGPPO_REQUIRE(n_desc >= 0 && n_desc <= DGPPO_GATHER_MAX, "gather_rows: n_desc must be in [0,%d] (got %d)", DGPPO_GATHER_MAX, n_desc);
  DGPPO_REQUIRE(n_ids >= 0, "gather_rows: negative n_ids");
  if (n_desc == 0 || n_ids == 0) return 0;
  DGPPO_REQUIRE(descs && ids, "gather_rows: NULL operand");
  DGPPO_REQUIRE(((uintptr_t)ids & 3) == 0, "gather_rows: ids must be 4-byte aligned");
  GatherArgs a{};
  long max_units = 0;
  for (int k = 0; k < n_desc; ++k) {
    const dgppo_gather_desc& d = descs[k];
    DGPPO_REQUIRE(d.src && d.dst, "gather_rows: NULL pointer in descriptor %d", k);
    DGPPO_REQUIRE(d.row_bytes > 0 && d.row_bytes % 4 == 0, "gather_rows: row_bytes of descriptor %d must be a positive multiple of 4 (got %lld)",
                  k, (long long)d.row_bytes);
    DGPPO_REQUIRE(d.src_stride >= 0 && d.src_stride % 4 == 0, "gather_rows: src_stride of descriptor %d must be a non-negative multiple of 4", k);
    DGPPO_REQUIRE(((uintptr_t)d.src & 3) == 0 && ((uintptr_t)d.dst & 3) == 0, "gather_rows: descriptor %d is not 4-byte aligned", k);
    a.src[k] = (const char*)d.src; a.dst[k] = (char*)d.dst; a.row_bytes[k] = d.row_bytes; a.src_stride[k] = d.src_stride;
    a.vec[k] = (d.row_bytes % 16 == 0 && d.src_stride % 16 == 0 && ((uintptr_t)d.src & 15) == 0 && ((uintptr_t)d.dst & 15) == 0) ? 1 : 0;
    const long units = a.vec[k] ? d.row_bytes >> 4 : d.row_bytes >> 2;
    max_units = units > max_units ? units : max_units;
  }
  a.ids = ids; a.n_ids = n_ids;
  // at most 64 workgroups along a row and 1024 id lanes: the loops take the rest
  const int gx = cdiv(max_units, 256) < 64 ? cdiv(max_units, 256) : 64;
  const int gy = n_ids < 1024 ? n_ids : 1024;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(gx, gy, n_desc), dim3(256), 0, (hipStream_t)stream, a);
  DGPPO_LAUNCH_CHECK();
  return 0;
}
