// les_hip_mem.h -- the one owner of the device and pinned-host allocations of the C ABI layer (les_hip.hip and its les_hip_*.inc
// parts).  Host-only; included by les_hip.hip after fail() / HIPCHECK and before the structs whose fields it owns; the same text in the
// gfx950 product, the plain check build and the CPU simulator build (LES_SIM).
//
// The rule: every hipMalloc / hipHostMalloc of that layer lives in a DevBuf / PinnedBuf -- as a struct field (freed with the struct,
// no list in a destroy function) or as a local (freed on every return path).  Kernel-argument structs stay plain and are filled from
// the owners' .p.  What deliberately stays raw:
//   - ViewData's members and the context's d_planes / planes_cap: les_hip_march.inc (frozen with the kernel headers, bench.py hashes
//     it) allocates straight into them; ~les_hip_ctx frees them.  ViewData itself stays a plain copyable aggregate without a destructor:
//     the simulator's launch macro captures its arguments' variables by value, and that file names `v.vol` of a `ViewData& v` in
//     launches -- a ViewData that freed on destruction would be freed by every such copy.  The two local DevBuf structs of
//     build_march_view and the d_img / d_hs unwinding of build_view in that file stay for the same reason (frozen).
//   - for the same capture rule, a launch never names an owner or a struct that holds one (PostScratch, UnaryTables, MtHost): it takes
//     `.p` through a pointer or a local raw copy.  The copy constructors are deleted, so the simulator build refuses a slip.
//   - memory handed across the C ABI (les_hip_malloc / les_hip_free, every void* / device address argument) belongs to the caller.
#pragma once

// Move-only owner of n elements of T in device memory (Pinned: in pinned host memory).  cap counts elements.
template <class T, bool Pinned = false> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;                        // (launches take .p, never the owner)
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }

    void reset()
    {
        if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p));
        p = nullptr; cap = 0;
    }
    // n elements (host_flags: hipHostMalloc's, pinned only); what the buffer held before is released first
    int alloc(size_t n, unsigned host_flags = hipHostMallocDefault)
    {
        reset();
        if (Pinned) HIPCHECK(hipHostMalloc((void**)&p, n * sizeof(T), host_flags));
        else HIPCHECK(hipMalloc((void**)&p, n * sizeof(T)));
        cap = n;
        return LES_HIP_OK;
    }
    // room for `need` elements, max(need, at_least) when it has to be made; the old contents are not kept
    int grow(size_t need, size_t at_least, hipStream_t stream, unsigned host_flags = hipHostMallocDefault)
    {
        if (need <= cap) return LES_HIP_OK;
        if (p) HIPCHECK(hipStreamSynchronize(stream));      // (launches in flight may still read the old buffer)
        return alloc(std::max(need, at_least), host_flags);
    }
    // pinned, allocated with hipHostMallocMapped: the address the device reaches the buffer at
    int dev(T** d) const
    {
#if defined(LES_SIM)
        *d = p;
#else
        HIPCHECK(hipHostGetDevicePointer((void**)d, p, 0));
#endif
        return LES_HIP_OK;
    }
};
template <class T> using PinnedBuf = DevBuf<T, true>;
