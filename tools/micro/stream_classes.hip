// Microbenchmark: does a stream priority class get hardware queues of its own?  ("few queues per class".)
// Eight non-blocking streams, four of normal priority and four of the greatest, an empty kernel on each.  Run it with
//   GPU_MAX_HW_QUEUES=4 AMD_LOG_LEVEL=4 ./stream_classes 2>&1 | grep "hardware queues with low priority"
// (the runtime counts its queues per class there), or under rocprofv3 --kernel-trace and read the Queue_Id column: one pool
// for all classes shows four ids, a pool per class eight.  Optional argument: kernels per stream (default 1).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ void k_empty() {}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 1;
    int least = 0, greatest = 0;
    CHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const char *q = getenv("GPU_MAX_HW_QUEUES");
    printf("GPU_MAX_HW_QUEUES %s, priority range: least %d, greatest %d\n", q ? q : "(unset)", least, greatest);
    hipStream_t s[8];
    for (int k = 0; k < 8; ++k) {
        if (k < 4) CHK(hipStreamCreateWithFlags(&s[k], hipStreamNonBlocking));
        else CHK(hipStreamCreateWithPriority(&s[k], hipStreamNonBlocking, greatest));
    }
    for (int r = 0; r < reps; ++r)
        for (int k = 0; k < 8; ++k) hipLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, s[k]);
    CHK(hipDeviceSynchronize());
    for (int k = 0; k < 8; ++k) {
        int p = 0;
        CHK(hipStreamGetPriority(s[k], &p));
        printf("stream %d: priority %d\n", k, p);
        CHK(hipStreamDestroy(s[k]));
    }
    return 0;
}
