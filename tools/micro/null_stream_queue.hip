// Microbenchmark: which calls give the process's null stream a hardware queue of its own?  ("few queues per
// class"; sibling of stream_classes.hip.)  Eight non-blocking streams, four of normal priority and four of the greatest, as the
// lanes of a pipeline under GPU_MAX_HW_QUEUES=4.  The first stream is created and used (an asynchronous upload, waited for) as
// epnn_create does; then ONE call chosen by the arm; then the other seven streams and `reps` empty kernels on each of the eight.
//   a        hipMemcpy (synchronous: it runs on the null stream)
//   b        nothing: the program only calls hipMalloc, hipMemcpyAsync on a created stream, hipStreamSynchronize and hipFree
//   c-free   hipMalloc + hipFree of a second buffer
//   c-event  hipEventRecord on the first stream + hipEventSynchronize
//   c-dsync  hipDeviceSynchronize
//   c-memset hipMemset (synchronous)
// Run every arm under rocprofv3 --kernel-trace and read Queue_Id per Stream_Id: eight ids = every stream has a queue of its own;
// seven = a normal queue belongs to the null stream and two normal streams share one.  Or with AMD_LOG_LEVEL=4 and
// grep "hardware queues with low priority": the runtime counts its queues per class each time it makes one.
//   GPU_MAX_HW_QUEUES=4 ./null_stream_queue ARM [reps]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ void k_empty() {}

int main(int argc, char **argv) {
    const char *arm = argc > 1 ? argv[1] : "b";
    const int reps = argc > 2 ? atoi(argv[2]) : 4;
    const char *arms[] = {"a", "b", "c-free", "c-event", "c-dsync", "c-memset"};
    bool known = false;
    for (const char *k : arms) known = known || !strcmp(arm, k);
    if (!known) { printf("unknown arm '%s' (a, b, c-free, c-event, c-dsync, c-memset)\n", arm); return 2; }
    int least = 0, greatest = 0;
    CHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const char *q = getenv("GPU_MAX_HW_QUEUES");
    printf("arm %s, GPU_MAX_HW_QUEUES %s, priority range: least %d, greatest %d\n", arm, q ? q : "(unset)", least, greatest);
    static float host[1024];
    float *dev = nullptr;
    CHK(hipMalloc(reinterpret_cast<void **>(&dev), sizeof(host)));
    hipStream_t s[8];
    CHK(hipStreamCreateWithFlags(&s[0], hipStreamNonBlocking));
    CHK(hipMemcpyAsync(dev, host, sizeof(host), hipMemcpyHostToDevice, s[0]));
    CHK(hipStreamSynchronize(s[0]));
    if (!strcmp(arm, "a")) CHK(hipMemcpy(dev, host, sizeof(host), hipMemcpyHostToDevice));
    if (!strcmp(arm, "c-free")) {
        float *tmp = nullptr;
        CHK(hipMalloc(reinterpret_cast<void **>(&tmp), sizeof(host)));
        CHK(hipFree(tmp));
    }
    if (!strcmp(arm, "c-event")) {
        hipEvent_t e;
        CHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        CHK(hipEventRecord(e, s[0]));
        CHK(hipEventSynchronize(e));
        CHK(hipEventDestroy(e));
    }
    if (!strcmp(arm, "c-dsync")) CHK(hipDeviceSynchronize());
    if (!strcmp(arm, "c-memset")) CHK(hipMemset(dev, 0, sizeof(host)));
    for (int k = 1; k < 8; ++k) {
        if (k < 4) CHK(hipStreamCreateWithFlags(&s[k], hipStreamNonBlocking));
        else CHK(hipStreamCreateWithPriority(&s[k], hipStreamNonBlocking, greatest));
    }
    for (int r = 0; r < reps; ++r)
        for (int k = 0; k < 8; ++k) hipLaunchKernelGGL(k_empty, dim3(1), dim3(64), 0, s[k]);
    for (int k = 0; k < 8; ++k) CHK(hipStreamSynchronize(s[k]));
    for (int k = 0; k < 8; ++k) CHK(hipStreamDestroy(s[k]));
    CHK(hipFree(dev));
    printf("done\n");
    return 0;
}
