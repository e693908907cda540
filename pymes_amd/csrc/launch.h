// The ordered host layer of the HIP units (kernels.hip, kernels_post.hip, kernels_integrals.hip, kernels_sector.hip).
//
// kernels.hip defers small launches in its phase queue.  Whatever is not recorded there -- a kernel launch of its own, a
// copy, a synchronisation, a graph boundary -- goes through the wrappers below, which launch the open phase first.  Below
// them the raw runtime names are poisoned: no unit that includes this header can bypass the layer.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#define HIP_CHECK(expr)                                                                   \
    do {                                                                                  \
        hipError_t err__ = (expr);                                                        \
        if (err__ != hipSuccess)                                                          \
            throw std::runtime_error(std::string("HIP error: ") + hipGetErrorString(err__) + \
                                     " at " __FILE__ ":" + std::to_string(__LINE__));     \
    } while (0)

namespace pymes_launch {
void phase_flush();      // launches what the calling thread's phase queue holds; defined in kernels.hip, next to the queue
}  // namespace pymes_launch

namespace {
using pymes_launch::phase_flush;

inline int grid_for(long total, int block = 256, int cap = 256 * 16) {
    long g = (total + block - 1) / block;
    return (int)std::max<long>(1, std::min<long>(g, cap));
}

// per device ordinal (a process may hold contexts on several GPUs)
constexpr int kMaxDevices = 16;
inline int current_device() {
    int d = 0;
    HIP_CHECK(hipGetDevice(&d));
    if (d < 0 || d >= kMaxDevices) throw std::runtime_error("device ordinal out of range");
    return d;
}
// a kernel's dynamic LDS limit, raised once per (kernel, device)
template <auto Kernel>
void allow_dynamic_lds(size_t bytes) {
    static bool done[kMaxDevices] = {false};
    const int dv = current_device();
    if (done[dv]) return;
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done[dv] = true;
}

// Every launch or stream operation below that is NOT recorded as a task goes through these: the open phase is launched
// first, so that the order of effects on the stream is that of immediate execution.  Below this block the raw runtime names
// are poisoned, and tests/test_capi_symbols.py refuses a raw kernel launch anywhere but here and in phase_flush.
template <typename... P, typename... A>
hipError_t try_launch_kernel(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
    phase_flush();
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    return hipGetLastError();
}
template <typename... P, typename... A>
void launch_kernel(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, const A&... args) {
    HIP_CHECK(try_launch_kernel(kernel, grid, block, lds, st, args...));
}
inline hipError_t copy_async(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
    phase_flush();
    return hipMemcpyAsync(dst, src, bytes, kind, st);
}
inline hipError_t set_async(void* dst, int value, size_t bytes, hipStream_t st) { phase_flush(); return hipMemsetAsync(dst, value, bytes, st); }
inline hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) { phase_flush(); return hipMemcpy(dst, src, bytes, kind); }
inline hipError_t sync_stream(hipStream_t st) { phase_flush(); return hipStreamSynchronize(st); }
inline hipError_t record_event(hipEvent_t ev, hipStream_t st) { phase_flush(); return hipEventRecord(ev, st); }
inline hipError_t wait_event(hipStream_t st, hipEvent_t ev, unsigned flags) { phase_flush(); return hipStreamWaitEvent(st, ev, flags); }
inline hipError_t launch_graph(hipGraphExec_t g, hipStream_t st) { phase_flush(); return hipGraphLaunch(g, st); }
inline hipError_t begin_capture(hipStream_t st, hipStreamCaptureMode mode) { phase_flush(); return hipStreamBeginCapture(st, mode); }
inline hipError_t end_capture(hipStream_t st, hipGraph_t* g) { phase_flush(); return hipStreamEndCapture(st, g); }
inline hipError_t free_device(void* p) { phase_flush(); return hipFree(p); }
#pragma GCC poison hipMemcpyAsync hipMemsetAsync hipMemcpy hipStreamSynchronize hipEventRecord hipStreamWaitEvent
#pragma GCC poison hipGraphLaunch hipStreamBeginCapture hipStreamEndCapture hipFree

inline void wait_idle(hipStream_t st) { HIP_CHECK(sync_stream(st)); }

}  // namespace
