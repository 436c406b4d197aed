// Staging of one host-pointer call in the context's arena (Ctx::d_stage). Plain C++, no HIP header: the library defines the five
// stage_* operations once (capi.hip, on the context's stream), tests/cpp/test_stage.cpp defines them as memcpy / logging no-ops and
// runs on the host compiler alone.
//
// A call declares its sections in order -- in() / out() / inout() with the host array and its element count, take() for a section
// only the device uses -- then upload() (reserve() + the declared host-to-device copies), at() / at_or_null() for the device
// pointers, its launches, and download() (the declared device-to-host copies + ONE synchronise). The byte count of every copy is
// sizeof(T) * count of the declaration, formed in note() and nowhere else. A null host array is carved like any other, copies nothing
// and reads as null through at_or_null(). Sections are 16-byte aligned and never overlap; the arena at least doubles when it grows.
// Invariant: every user copies into, launches on and reads back from the arena on c->stream only, so successive calls are ordered by
// that stream (the entries that return before their kernel has read the arena -- hv_ingest_build, the EKF's predict / update /
// augment forms -- included); growth drains c->stream before it frees, and hv_set_stream drains the old stream before it swaps. A
// forked visit (ekf_visit.hip) reads uploaded sections on aux_stream, but joins c->stream again inside the visit, in front of the
// entry's download and synchronise.
#pragma once
#include <stddef.h>

#include "../../include/hybvio_hip.h"
#include "dev_buf.hpp"

namespace hv { struct Ctx; }

// (hidden: the library exports its C entry points, not its plumbing)
#pragma GCC visibility push(hidden)
namespace hv {

DevBuf<unsigned char> &stage_arena(Ctx *c);                                       // Ctx::d_stage (count() = its bytes)
int stage_drain(Ctx *c);                                                          // everything on c->stream has finished (before growth frees)
int stage_to_device(Ctx *c, void *dst_dev, const void *src_host, size_t bytes);   // asynchronous, on c->stream
int stage_to_host(Ctx *c, void *dst_host, const void *src_dev, size_t bytes);     // asynchronous, on c->stream
int stage_sync(Ctx *c);                                                           // c->stream has finished

template <class T> struct StageSection { size_t off; bool bound; };               // bound: declared with a host array (take(): always)

struct Stage {
    static constexpr int MAX_COPIES = 12;                  // (the largest users, the EKF frame loops and the hybrid visit, declare 10)
    struct Copy { size_t off, bytes; const void *up; void *down; };
    Ctx *c; size_t total = 0;
    Copy copies[MAX_COPIES]; int n_copies = 0; bool overflow = false;
    explicit Stage(Ctx *ctx) : c(ctx) {}

    template <class T> StageSection<T> take(size_t count) { return carve<T>(count, true); }
    template <class T> StageSection<T> in(const T *host, size_t count) { return note<T>(count, host, nullptr); }
    template <class T> StageSection<T> out(T *host, size_t count) { return note<T>(count, nullptr, host); }
    template <class T> StageSection<T> inout(T *host, size_t count) { return note<T>(count, host, host); }

    int reserve()
    {
        const size_t have = stage_arena(c).count();
        if (total <= have) return HV_OK;
        return grow_buffers([this] { return stage_drain(c); }, {{stage_arena(c), total > 2 * have ? total : 2 * have}});
    }
    int upload()
    {
        if (overflow) return HV_ERR_INVALID;
        if (const int rc = reserve()) return rc;
        for (int i = 0; i < n_copies; ++i)
            if (copies[i].up) if (const int rc = stage_to_device(c, stage_arena(c) + copies[i].off, copies[i].up, copies[i].bytes)) return rc;
        return HV_OK;
    }
    int download()
    {
        if (overflow) return HV_ERR_INVALID;
        for (int i = 0; i < n_copies; ++i)
            if (copies[i].down) if (const int rc = stage_to_host(c, copies[i].down, stage_arena(c) + copies[i].off, copies[i].bytes)) return rc;
        return stage_sync(c);
    }
    // a download whose size came back from the device: the first `count` elements of a section, now, without a synchronise
    template <class T> int fetch(T *host, StageSection<T> s, size_t count) { return stage_to_host(c, host, at(s), sizeof(T) * count); }
    int sync() { return stage_sync(c); }

    template <class T> T *at(StageSection<T> s) const { return reinterpret_cast<T *>(stage_arena(c) + s.off); }
    template <class T> T *at_or_null(StageSection<T> s) const { return s.bound ? at(s) : nullptr; }

private:
    template <class T> StageSection<T> carve(size_t count, bool bound)
    {
        const StageSection<T> s{total, bound};
        total += (count * sizeof(T) + 15) & ~(size_t)15;
        return s;
    }
    template <class T> StageSection<T> note(size_t count, const T *up, T *down)
    {
        const StageSection<T> s = carve<T>(count, up || down);
        if (!s.bound || count == 0) return s;
        if (n_copies == MAX_COPIES) { overflow = true; return s; }
        copies[n_copies++] = Copy{s.off, sizeof(T) * count, up, down};
        return s;
    }
};

}  // namespace hv
#pragma GCC visibility pop
