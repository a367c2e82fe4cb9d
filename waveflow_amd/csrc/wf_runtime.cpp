// wf_runtime.cpp -- HIP error state, per-kernel LDS attributes, the model's device allocations and the model-free parts of the C ABI.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "wf_model.h"

namespace wf {

static thread_local int g_last_hip = 0;
void set_hip_error(int e) { g_last_hip = e; }

int ensure_dynamic_lds(const void* kernel, int lds_bytes, DynLdsSlots* slots) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) dev = -1;
    int* slot = dev >= 0 ? &slots->bytes[dev] : nullptr;
    const int have = slot ? __atomic_load_n(slot, __ATOMIC_RELAXED) : 0;
    if (slot && lds_bytes <= have) return WF_OK;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) {
        set_hip_error((int)e);
        return WF_ERR_HIP;
    }
    if (slot) {   // keep the maximum (another thread may have stored a larger request meanwhile)
        int cur = have;
        while (cur < lds_bytes && !__atomic_compare_exchange_n(slot, &cur, lds_bytes, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
    return WF_OK;
}

int dev_alloc_bytes(wf_model* m, void** p, size_t bytes) {
    void* q = nullptr;
    WF_HIP(hipMalloc(&q, bytes));
    // WF_POISON=1 (the test suite sets it): fresh device memory starts as NaN patterns, so that a kernel reading anything
    // it or the host has not written shows up as NaN instead of passing by luck on zero-filled pages
    if (env_poison()) (void)hipMemset(q, 0xFF, bytes);
    m->allocs.push_back(q);
    *p = q;
    return WF_OK;
}

// grows the model's private device scratch (tails of the wave kernels when the caller passes no workspace)
int ensure_scratch(const wf_model* cm, int64_t floats) {
    wf_model* m = const_cast<wf_model*>(cm);
    if (m->scratch_floats >= floats) return WF_OK;
    if (m->d_scratch) {
        WF_HIP(hipDeviceSynchronize());
        (void)hipFree(m->d_scratch);
        m->allocs.erase(std::remove(m->allocs.begin(), m->allocs.end(), (void*)m->d_scratch), m->allocs.end());
        m->d_scratch = nullptr;
        m->scratch_floats = 0;
    }
    int rc = dev_alloc(m, &m->d_scratch, (size_t)floats);
    if (rc) return rc;
    m->scratch_floats = floats;
    return WF_OK;
}

}  // namespace wf

using namespace wf;

extern "C" {

int wf_abi_version(void) { return WF_ABI_VERSION; }

const char* wf_strerror(int status) {
    switch (status) {
        case WF_OK: return "ok";
        case WF_ERR_INVALID: return "invalid argument";
        case WF_ERR_UNSUPPORTED: return "configuration not supported by this build";
        case WF_ERR_HIP: return "HIP runtime error (see wf_last_hip_error_string)";
        case WF_ERR_NO_DEVICE: return "no gfx950 device available (there is no CPU fallback)";
        case WF_ERR_NOMEM: return "out of memory";
        case WF_ERR_NUMERIC: return "numerical failure while building tables";
        default: return "unknown status";
    }
}

int wf_last_hip_error(void) { return g_last_hip; }
const char* wf_last_hip_error_string(void) { return hipGetErrorString((hipError_t)g_last_hip); }

int wf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int good = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && std::string(p.gcnArchName).rfind("gfx950", 0) == 0) ++good;
    }
    return good;
}

int wf_tables_build(int kind, int degree, int n_internal_knots, int n_mesh, double* out, double* b_to_ob, double* ob_to_b) {
    if (kind < WF_SPLINE_M || kind > WF_SPLINE_OB) return WF_ERR_INVALID;
    if (degree < 1 || n_internal_knots < 2 || n_mesh < 2) return WF_ERR_INVALID;
    const int nb = n_bases_of(kind, degree, n_internal_knots);
    if (!out) return nb;
    if (kind != WF_SPLINE_OB) return build_raw_table(kind, degree, n_internal_knots, n_mesh, out);
    std::vector<double> b64;
    try {
        b64.resize((size_t)4 * nb * n_mesh);
    } catch (const std::bad_alloc&) {
        return WF_ERR_NOMEM;
    }
    int rc = build_raw_table(WF_SPLINE_B, degree, n_internal_knots, n_mesh, b64.data());
    if (rc < 0) return rc;
    return build_ortho_b(degree, n_internal_knots, n_mesh, b64.data(), out, b_to_ob, ob_to_b);
}

}  // extern "C"
