// lhip_rt.h -- what the host side stands on: the per-thread error and statistics state, set_err, HIPCK and the rt:: runtime shim
// (HIP for the product; plain host memory for the CPU simulations, -DLHIP_HOSTSIM).
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// ===========================================================================================
// runtime shim
// ===========================================================================================
static thread_local std::string g_err;
static thread_local int64_t g_stat_frames = 0, g_stat_repaired = 0, g_stat_iters = 0;
// profiling counters of the dev builds (tests/tools/phase_prof.py, wave_tail.py); the product only allocates and zeroes them
#if defined(LHIP_PHASE_PROF) || defined(LHIP_WAVE_TIMES)
enum { PROF_BYTES = 512 + 16 * 8192 + 512 };   /* + (start, end) of every wave of the last g_quant launch (100 MHz ticks): the launch's tail; + the stage stamps of g_frame */
enum { FRAME_PROF_BASE = 64 + 2 * 8192 };      /* u64 index of g_frame's stage stamps */
#else
enum { PROF_BYTES = 512 };
#endif
struct Context;
static thread_local Context* g_rej_pending = nullptr;       // the last batch counted rejected Float32 samples on the device (lhip_last_batch_rejected_samples fetches the count)
static thread_local int64_t g_rejected = 0;
static thread_local uint32_t g_last_paths = 0;              // launch decisions of the last batch (LHIP_PATH_* of include/lamejs_hip.h; lhip_debug_last_paths)
// the speculative quantization launch of the last batch (lhip_debug_read(11), a test hook): all zero when the batch launched none (one-frame program, reservoir).
// kernel: 1 g_quant_fast, 2 g_quant_pair, 3 g_quant; pair / skip: the PAIR and SKIP template arguments (g_quant_pair: pair = 1, g_quant: pair = 0)
struct QuantLaunch { int32_t workgroups = 0, waves = 0, nfs = 0, kernel = 0, pair = 0, skip = 0, pad_[2] = {0, 0}; };
enum { QL_FAST = 1, QL_PAIR = 2, QL_PERSISTENT = 3 };
static thread_local QuantLaunch g_last_quant;
static thread_local Context* g_stat_pending = nullptr;      // the last batch was enqueued without synchronisation: its repair statistics are still on the device
static void set_err(const std::string& e) { g_err = e; }

#ifdef LHIP_HOSTSIM
namespace rt {
// LHIP_HOSTSIM_DEVICES=n (tests): the simulation pretends to have n devices -- one Context each, so that lhip_set_devices' round-robin
// placement, lhip_stream_device and host threads batching on different contexts at the same time run in the CPU tier (ASan / TSan)
static int device_count() { static const int n = []() { const char* e = getenv("LHIP_HOSTSIM_DEVICES"); const int v = e ? atoi(e) : 1; return v >= 1 && v <= 64 ? v : 1; }(); return n; }
static bool set_device(int) { return true; }
static void* dmalloc(size_t n) { return calloc(1, n ? n : 1); }
static void dfree(void* p) { free(p); }
static bool h2d(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); return true; }
static bool d2h(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); return true; }
static bool d2d(void* d, const void* s, size_t n, void*) { memmove(d, s, n); return true; }
static bool dzero(void* d, size_t n, void*) { memset(d, 0, n); return true; }
static bool sync(void*) { return true; }
// streams and events of the chunked host path: everything is synchronous here, so ordering holds trivially
static bool stream_create(void** s) { *s = (void*)(uintptr_t)1; return true; }
static bool event_create(void** e) { *e = (void*)(uintptr_t)1; return true; }
static bool event_record(void*, void*) { return true; }
static bool stream_wait_event(void*, void*) { return true; }
static void* host_alloc_pinned(size_t n) { return calloc(1, n ? n : 1); }
static void host_free_pinned(void* p) { free(p); }
}  // namespace rt
#else
#define HIPCK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { set_err(std::string(#x) + ": " + hipGetErrorString(e_)); return false; } } while (0)
namespace rt {
// LHIP_ALIAS_DEVICES=n (tests only, 2 <= n <= 8): ordinals 0 .. n-1 are n SEPARATE library contexts -- own mutex, own HIP stream, own workspaces, own table
// uploads -- on physical device 0, so that a box with one GPU runs the multi-device paths (lhip_set_devices' round-robin placement, host threads batching
// on two contexts at the same time) against real HIP (tests/test_gpu_parity.py::test_gpu_two_devices_*).  Read at every call: a test sets it for its own duration.
static int alias_n() { const char* e = getenv("LHIP_ALIAS_DEVICES"); const int v = e ? atoi(e) : 0; return v >= 2 && v <= 8 ? v : 0; }
static int phys(int d) { return alias_n() ? 0 : d; }
static int device_count() { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; const int a = alias_n(); return (a && n >= 1) ? a : n; }
static bool set_device(int d) { HIPCK(hipSetDevice(phys(d))); return true; }
static void* dmalloc(size_t n) { void* p = nullptr; if (hipMalloc(&p, n ? n : 1) != hipSuccess) return nullptr; return p; }
static void dfree(void* p) { if (p) (void)hipFree(p); }
static bool h2d(void* d, const void* s, size_t n, void* st) { if (n) HIPCK(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, (hipStream_t)st)); return true; }
static bool d2h(void* d, const void* s, size_t n, void* st) { if (n) HIPCK(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, (hipStream_t)st)); return true; }
static bool d2d(void* d, const void* s, size_t n, void* st) { if (n) HIPCK(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, (hipStream_t)st)); return true; }
static bool dzero(void* d, size_t n, void* st) { if (n) HIPCK(hipMemsetAsync(d, 0, n, (hipStream_t)st)); return true; }
static bool sync(void* st) { HIPCK(hipStreamSynchronize((hipStream_t)st)); return true; }
static bool stream_create(void** s) { hipStream_t t; HIPCK(hipStreamCreateWithFlags(&t, hipStreamNonBlocking)); *s = t; return true; }
static bool event_create(void** e) { hipEvent_t t; HIPCK(hipEventCreateWithFlags(&t, hipEventDisableTiming)); *e = t; return true; }
static bool event_record(void* e, void* st) { HIPCK(hipEventRecord((hipEvent_t)e, (hipStream_t)st)); return true; }
static bool stream_wait_event(void* st, void* e) { HIPCK(hipStreamWaitEvent((hipStream_t)st, (hipEvent_t)e, 0)); return true; }
static void* host_alloc_pinned(size_t n) { void* p = nullptr; if (hipHostMalloc(&p, n ? n : 1, hipHostMallocDefault) != hipSuccess) return nullptr; return p; }
static void host_free_pinned(void* p) { if (p) (void)hipHostFree(p); }
}  // namespace rt
#endif
