// weights.h — staging and upload of one state dict: what the seven loaders / finalizers of the fp16 engine (engine_pack.hip, T = f16)
// and of the fp32 net (f32_pack.hip, T = float) share.  A loader normalises the tensor's name and calls stage_tensor(); a finalizer
// packs the staged tensors into a host blob (WeightSet::get marks what it consumed) and hands the blob to WeightSet::finish().
#pragma once
#include "../../include/dm_engine.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <type_traits>
#include <vector>
#include <hip/hip_runtime.h>

namespace dm {

template <class T> struct HostTensorT {
    std::vector<T> data;
    std::vector<int64_t> shape;
    bool used = false;
    size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};
template <class T> using TensorMap = std::map<std::string, HostTensorT<T>>;

// host_ptr [shape] of DM_F16 or DM_F32 -> map[name] in T (copied, or converted element by element: (f16)float, (float)_Float16).
// A caller that stores a tensor under fewer dimensions (the VAE's legacy [C, C, 1, 1] projections) passes the smaller ndim.
template <class T>
int stage_tensor(TensorMap<T>& map, const std::string& name, const void* host_ptr, int dtype, const int64_t* shape, int ndim, std::string& err) {
    constexpr bool f32 = std::is_same<T, float>::value;
    using Other = typename std::conditional<f32, _Float16, float>::type;
    char msg[512];
    if (ndim < 0 || ndim > 8) { snprintf(msg, sizeof(msg), "bad ndim %d for %s", ndim, name.c_str()); err = msg; return 1; }
    HostTensorT<T> t;
    t.shape.assign(shape, shape + ndim);
    const size_t n = t.numel();
    t.data.resize(n);
    if (dtype == (f32 ? DM_F32 : DM_F16)) memcpy(t.data.data(), host_ptr, n * sizeof(T));
    else if (dtype == (f32 ? DM_F16 : DM_F32)) { const Other* o = (const Other*)host_ptr; for (size_t i = 0; i < n; ++i) t.data[i] = (T)o[i]; }
    else { snprintf(msg, sizeof(msg), "unsupported dtype %d for %s", dtype, name.c_str()); err = msg; return 1; }
    map[name] = std::move(t);
    return 0;
}

// What belongs to one state dict: the tensors staged on the host, then the device slab they were packed into.
template <class T> struct WeightSet {
    TensorMap<T> host;
    T* slab = nullptr; size_t bytes = 0;
    bool ready = false;

    HostTensorT<T>* get(const std::string& name, std::initializer_list<int64_t> shape, std::string& err) {
        auto it = host.find(name);
        if (it == host.end()) { err = "missing tensor: " + name; return nullptr; }
        HostTensorT<T>& t = it->second;
        const std::vector<int64_t> want(shape);
        if (t.shape != want) {
            err = "shape mismatch for " + name + ": got [";
            for (auto v : t.shape) err += std::to_string(v) + ",";
            err += "] want [";
            for (auto v : want) err += std::to_string(v) + ",";
            err += "]";
            return nullptr;
        }
        t.used = true;
        return &t;
    }
    // The tail of a finalize: every staged tensor consumed, `expected` of them (0: any number), blob -> a new device slab, staging
    // released, ready.  A failure changes nothing: the set stays un-ready, keeps its tensors and can be loaded and finalized again.
    int finish(const void* blob, size_t blob_bytes, const char* what, size_t expected, std::string& err) {
        char msg[768];
        size_t unused = 0; const char* first = "";
        for (auto& kv : host) if (!kv.second.used) { if (!unused) first = kv.first.c_str(); ++unused; }
        if (unused) { snprintf(msg, sizeof(msg), "%zu unexpected tensors in the %s state dict (first: %s)", unused, what, first); err = msg; return 1; }
        if (expected && host.size() != expected) {
            snprintf(msg, sizeof(msg), "expected %zu %s tensors, got %zu", expected, what, host.size()); err = msg; return 1;
        }
        T* dev = nullptr;
        hipError_t r = hipMalloc((void**)&dev, blob_bytes);
        if (r == hipSuccess) r = hipMemcpy(dev, blob, blob_bytes, hipMemcpyHostToDevice);
        if (r != hipSuccess) {
            if (dev) (void)hipFree(dev);
            snprintf(msg, sizeof(msg), "upload of the %s weights (%zu bytes) failed: %s", what, blob_bytes, hipGetErrorString(r)); err = msg; return 1;
        }
        if (slab) (void)hipFree(slab);         // finalized again after a later step of the caller's finalize failed
        slab = dev; bytes = blob_bytes;
        host.clear();
        ready = true;
        return 0;
    }
};

}  // namespace dm
