// Diagnostic: what a dependent kernel boundary costs when the predecessor
// leaves B bytes of freshly stored lines behind, and what a store policy does
// to it and to the next launch's loads.  A chain of two alternating kernels on
// one stream, 256 workgroups x 256 threads each:
//   writer: workgroup g stores chunk g (B / 256 bytes, 16 B per lane per
//           store) with plain, write-through (two 8-byte relaxed agent-scope
//           atomic stores: sc1), non-temporal (nt) or one 16-byte write-through
//           buffer store (sc1x16) stores;
//   reader: workgroup g loads chunk g (the workgroup that wrote it: same XCD,
//           workgroups go round-robin over the 8 XCDs), chunk g + 1 (written
//           on the next XCD), or nothing ("none": the writer and its boundary
//           alone).
// B = 0, 2.7, 7.5, 12.6, 25 MB: the per-launch write volumes of the C3 step's
// CR stages (profiles/r06_pmc_traffic.json).  Prints us per launch pair.
// Build: hipcc --offload-arch=gfx950 -O3 boundary_dirty.hip -o boundary_dirty
#include <hip/hip_runtime.h>
#include <cstdio>

typedef double v2d __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

enum { PLAIN = 0, THROUGH = 1, STREAM = 2, THROUGH16 = 3 };

template <int POL>
__device__ __forceinline__ void st16(double2* p, double2 v) {
  if constexpr (POL == THROUGH) {
    double* q = reinterpret_cast<double*>(p);
    __hip_atomic_store(q, v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(q + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else if constexpr (POL == STREAM) {
    __builtin_nontemporal_store(v2d{v.x, v.y}, reinterpret_cast<v2d*>(p));
  } else {
    *p = v;
  }
}

// chunk: double2 elements per workgroup
template <int POL>
__global__ __launch_bounds__(256) void k_write(double2* __restrict__ buf, int chunk, double x) {
  if constexpr (POL == THROUGH16) {
    // the whole buffer as one raw buffer (stores past nbytes are dropped); aux 16 = sc1
    const unsigned nbytes = gridDim.x * (unsigned)chunk * 16u;
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(buf, 0, (int)nbytes, 0x00020000);
    for (int i = threadIdx.x; i < chunk; i += 256)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, make_double2(x, (double)i)), r,
                                             (int)((blockIdx.x * (unsigned)chunk + i) * 16u), 0, 16);
  } else {
    double2* c = buf + (size_t)blockIdx.x * chunk;
    for (int i = threadIdx.x; i < chunk; i += 256) st16<POL>(c + i, make_double2(x, (double)i));
  }
}

// rot: the reader's chunk is rot workgroups (= XCDs) ahead of its own; n: elements read
__global__ __launch_bounds__(256) void k_read(const double2* __restrict__ buf, int chunk, int n, int rot,
                                              double* __restrict__ sink) {
  const double2* c = buf + (size_t)((blockIdx.x + rot) % gridDim.x) * chunk;
  double a = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double2 v = c[i];
    a += v.x + v.y;
  }
  if (a == 12345.678) sink[blockIdx.x] = a;   // never true: keeps the loads
}

int main() {
  const int WG = 256, K = 400;
  const double mbs[5] = {0.0, 2.7, 7.5, 12.6, 25.0};
  const int maxchunk = (int)(25.0e6 / 16 / WG) + 1;
  double2* buf;
  double* sink;
  if (hipMalloc(&buf, (size_t)WG * maxchunk * sizeof(double2)) != hipSuccess) return 1;
  if (hipMalloc(&sink, WG * sizeof(double)) != hipSuccess) return 1;
  (void)hipMemset(buf, 0, (size_t)WG * maxchunk * sizeof(double2));
  hipStream_t s;
  (void)hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  const char* pname[4] = {"plain", "sc1", "nt", "sc1x16"};
  const char* rname[3] = {"same-xcd", "next-xcd", "none"};
  printf("%8s %6s %9s %12s\n", "MB", "store", "reader", "us/pair");
  for (int rep = 0; rep < 2; ++rep)   // the second pass shows the run-to-run spread
    for (int b = 0; b < 5; ++b) {
      const int chunk = (int)(mbs[b] * 1e6 / 16 / WG);   // <= maxchunk
      for (int pol = 0; pol < 4; ++pol)
        for (int rd = 0; rd < 3; ++rd) {
          auto pair = [&](int k) {
            const double x = (double)k;
            if (pol == PLAIN) hipLaunchKernelGGL(k_write<PLAIN>, dim3(WG), dim3(256), 0, s, buf, chunk, x);
            else if (pol == THROUGH) hipLaunchKernelGGL(k_write<THROUGH>, dim3(WG), dim3(256), 0, s, buf, chunk, x);
            else if (pol == STREAM) hipLaunchKernelGGL(k_write<STREAM>, dim3(WG), dim3(256), 0, s, buf, chunk, x);
            else hipLaunchKernelGGL(k_write<THROUGH16>, dim3(WG), dim3(256), 0, s, buf, chunk, x);
            hipLaunchKernelGGL(k_read, dim3(WG), dim3(256), 0, s, buf, chunk, rd == 2 ? 0 : chunk, rd == 1 ? 1 : 0,
                               sink);
          };
          for (int k = 0; k < 20; ++k) pair(k);
          (void)hipEventRecord(e0, s);
          for (int k = 0; k < K; ++k) pair(k);
          (void)hipEventRecord(e1, s);
          if (hipEventSynchronize(e1) != hipSuccess) {
            printf("device error: %s\n", hipGetErrorString(hipGetLastError()));
            return 1;
          }
          float ms = 0;
          (void)hipEventElapsedTime(&ms, e0, e1);
          printf("%8.1f %6s %9s %12.2f\n", mbs[b], pname[pol], rname[rd], 1000.0 * ms / K);
        }
    }
  return 0;
}
