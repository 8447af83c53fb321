// In which steps does the hardware hand out LDS to a workgroup?  Single-wave workgroups with s bytes of dynamic LDS count how many of them are resident at once:
// every workgroup adds itself to a counter, keeps the maximum it saw, waits 0.5 ms and leaves.  With few registers the wave slots allow 32 workgroups per compute unit,
// so above 160 KB / 32 = 5 120 B the LDS decides, and resident / CUs = floor(160 KB / allocation(s)) shows the allocation as a staircase in s.
//   hipcc --offload-arch=gfx950 -O3 tools/lds_granule_probe.hip -o tools/lds_granule_probe && tools/lds_granule_probe
#include <hip/hip_runtime.h>
#include <cstdio>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ __launch_bounds__(64) void k_resident(int* active, int* peak, long long ticks) {
    extern __shared__ unsigned dyn[];
    dyn[threadIdx.x] = threadIdx.x;
    if (threadIdx.x == 0) {
        const int now = atomicAdd(active, 1) + 1;
        atomicMax(peak, now);
        const long long t0 = wall_clock64();
        while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
        atomicSub(active, 1);
    }
}

int main() {
    hipDeviceProp_t pr;
    CK(hipGetDeviceProperties(&pr, 0));
    const int cus = pr.multiProcessorCount;
    int* d;
    CK(hipMalloc(&d, 2 * sizeof(int)));
    printf("%s: %d CUs, %zu B LDS per workgroup at most\n", pr.gcnArchName, cus, (size_t)pr.sharedMemPerBlock);
    printf("%8s %10s %8s %12s\n", "bytes", "resident", "per CU", "160K/perCU");
    int last = -1;
    for (int s = 4096; s <= 8192; s += 64) {
        CK(hipMemset(d, 0, 2 * sizeof(int)));
        hipLaunchKernelGGL(k_resident, dim3(cus * 40), dim3(64), s, 0, d, d + 1, 50000ll);      // 100 MHz clock: 0.5 ms; 40 per CU: more than can be resident
        CK(hipDeviceSynchronize());
        int h[2];
        CK(hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost));
        const int per = h[1] / cus;
        if (per != last) printf("%8d %10d %8d %12d\n", s, h[1], per, per ? 163840 / per : 0);
        last = per;
    }
    CK(hipFree(d));
    return 0;
}
