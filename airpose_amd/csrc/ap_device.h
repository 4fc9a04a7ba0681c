// Per-device launch-side state of libairpose_hip.so: host code only, no kernel.
//
// hipFuncSetAttribute and the CU count are per DEVICE: whatever a launcher caches about them is keyed by the current device id
// (two nets of one process on two GPUs, e.g. copenet_sep, each get their >64 KiB dynamic-LDS opt-in).  Handles on different
// threads work, so the caches are atomics: a launch that has been made before costs hipGetDevice and one acquire load, there is
// no mutex, and two threads racing through a first call may both do the (idempotent) work.  A failure is returned and NOT cached:
// the next launch tries again.  DESIGN.md, "Per-device launch state".
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <initializer_list>

#define AP_MAX_DEVICES 16

// the library's own: one copy for all its translation units, none in its dynamic symbol table
#define AP_LIBRARY_WIDE __attribute__((visibility("hidden"))) inline

// CU count per device; 0 = not yet asked
AP_LIBRARY_WIDE std::atomic<int> ap_cu_count[AP_MAX_DEVICES];

// the current device id (< AP_MAX_DEVICES) and, with a non-null n_cu, its CU count; a count <= 0 is hipErrorInvalidDevice, so
// that no launcher has to decide what a grid sized by it would mean
static inline hipError_t ap_device(int* dev, int* n_cu) {
    hipError_t e = hipGetDevice(dev);
    if (e != hipSuccess) return e;
    if (*dev < 0 || *dev >= AP_MAX_DEVICES) return hipErrorInvalidDevice;
    if (!n_cu) return hipSuccess;
    int n = ap_cu_count[*dev].load(std::memory_order_relaxed);
    if (!n) {
        e = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, *dev);
        if (e != hipSuccess) return e;
        if (n <= 0) return hipErrorInvalidDevice;
        ap_cu_count[*dev].store(n, std::memory_order_relaxed);
    }
    *n_cu = n;
    return hipSuccess;
}

// 256 bytes of zeros on the current device (the DMA source of predicated-off rows), allocated on first use and kept for the
// process.  The pointer is published by a compare-exchange: of two threads racing through the first call the loser frees its own
// line and takes the winner's
AP_LIBRARY_WIDE std::atomic<void*> ap_zero[AP_MAX_DEVICES];

static inline hipError_t ap_zero_line(const void** out) {
    int dev = 0;
    hipError_t e = ap_device(&dev, nullptr);
    if (e != hipSuccess) return e;
    void* z = ap_zero[dev].load(std::memory_order_acquire);
    if (!z) {
        e = hipMalloc(&z, 256);
        if (e != hipSuccess) return e;
        e = hipMemset(z, 0, 256);
        void* winner = nullptr;
        if (e != hipSuccess || !ap_zero[dev].compare_exchange_strong(winner, z, std::memory_order_acq_rel, std::memory_order_acquire)) {
            (void)hipFree(z);
            if (e != hipSuccess) return e;
            z = winner;
        }
    }
    *out = z;
    return hipSuccess;
}

// "f has succeeded on this device": zero-initialisable, one `static ApDeviceOnce` per launcher (per instantiation of a template)
struct ApDeviceOnce { std::atomic<unsigned char> done[AP_MAX_DEVICES]; };

template <class F>
hipError_t ap_once_per_device(ApDeviceOnce& once, int dev, F&& f) {
    if (once.done[dev].load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = f();
    if (e == hipSuccess) once.done[dev].store(1, std::memory_order_release);
    return e;
}

// a kernel and the dynamic LDS it is launched with
struct ApLdsKernel {
    const void* kernel;
    int bytes;
    template <class K> ApLdsKernel(K* k, int b) : kernel((const void*)k), bytes(b) {}
};

// once per device: allow each kernel named its own amount of dynamic LDS (more than the 64 KiB a kernel gets unasked)
static inline hipError_t ap_lds_optin(ApDeviceOnce& once, int dev, std::initializer_list<ApLdsKernel> kernels) {
    return ap_once_per_device(once, dev, [&]() -> hipError_t {
        for (const ApLdsKernel& k : kernels) {
            const hipError_t e = hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    });
}
