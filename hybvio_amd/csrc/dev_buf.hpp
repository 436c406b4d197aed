// Owning device buffers. Plain C++, no HIP header: the library defines dev_alloc / dev_free once (capi.hip: hipMalloc / hipFree),
// tests/cpp/test_dev_buf.cpp defines them as a counting allocator and runs on the host compiler alone.
#pragma once
#include <stddef.h>
#include <initializer_list>

#include "../../include/hybvio_hip.h"

namespace hv {

int dev_alloc(void **p, size_t bytes);   // HV_OK, or HV_ERR_NOMEM with *p left null
void dev_free(void *p);                  // p != null

// the untyped part of a DevBuf: the block and the element count it was allocated for
class DevMem {
public:
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { reset(); }
    void reset()
    {
        if (p_) dev_free(p_);
        p_ = nullptr; n_ = 0;
    }
    size_t count() const { return n_; }
protected:
    DevMem(DevMem &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    void take(DevMem &o)
    {
        if (this == &o) return;
        reset();
        p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0;
    }
    int alloc_bytes(size_t count, size_t elem)
    {
        reset();
        if (dev_alloc(&p_, count * elem) != HV_OK) { p_ = nullptr; return HV_ERR_NOMEM; }
        n_ = count;
        return HV_OK;
    }
    void *p_ = nullptr;
    size_t n_ = 0;
    friend struct GrowSlot;
};

// `count` elements of T on the device. Move-only; converts to T * wherever a kernel argument or a copy wants the pointer.
template <class T> class DevBuf : public DevMem {
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : DevMem(static_cast<DevMem &&>(o)) {}
    DevBuf &operator=(DevBuf &&o) noexcept { take(o); return *this; }
    int alloc(size_t count) { return alloc_bytes(count, sizeof(T)); }   // frees what it holds first; on failure the buffer is empty
    int alloc_once(size_t count) { return p_ ? (int)HV_OK : alloc(count); }   // members of a group that never grow
    T *get() const { return static_cast<T *>(p_); }
    operator T *() const { return get(); }
};

// one member of a group that grows together, and the element count it is to have
struct GrowSlot {
    DevMem *buf; size_t count, elem;
    template <class T> GrowSlot(DevBuf<T> &b, size_t n) : buf(&b), count(n), elem(sizeof(T)) {}
    int alloc() const { return buf->alloc_bytes(count, elem); }
};

// Growing a group of device buffers: drain() (everything that may still read the old blocks; a non-zero return ends the call with
// nothing freed), then frees every member, then allocates them again at their new counts. The caller tests whether growth is needed,
// zeroes the group's capacity field before the call and sets it after an HV_OK, so that a failure in the middle -- the members in
// front of it allocated, the others empty -- leaves a group that reads as empty.
template <class Drain> int grow_buffers(Drain &&drain, std::initializer_list<GrowSlot> slots)
{
    if (const int rc = drain()) return rc;
    for (const GrowSlot &g : slots) g.buf->reset();
    for (const GrowSlot &g : slots) if (const int rc = g.alloc()) return rc;
    return HV_OK;
}

}  // namespace hv
