// sx_hostio.hpp -- what the streaming writer (sx_build.hip), the index (sx_index.hip) and the mapper (sx_sam.hip) share: the
// context's two pinned staging buffers, the chunked copies through them (sx_hostio.hip), the owner of a call's hipMallocs.
#pragma once
#include "sx_common.hpp"

#include <algorithm>

// The only place that allocates ctx->h_stage[0 .. 1] (SX_STAGE_BYTES each, kept until the context goes); SX_E_NOMEM: a
// buffer whose allocation fails stays null and is tried again by the next call
int sx_stage_ensure(sx_ctx *ctx);
// device -> sink in chunks of at most SX_STAGE_BYTES: the copy of chunk k + 1 runs while the sink (typically fwrite)
// works on chunk k; nothing of the array's size exists on the host
int sx_stream_to_sink(sx_ctx *ctx, int section, const void *d_src, size_t bytes, sx_sink_fn sink, void *user);
// host -> device in the same chunks: the copy of a chunk runs while the host fills the next one
int sx_upload_staged(sx_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);

static inline int sx_nomem_of(int rc) { return rc == (int)hipErrorOutOfMemory ? SX_E_NOMEM : rc; }

// one event a staging buffer: recorded behind the buffer's copy, waited for before the buffer is touched again
struct sx_stage_events {
    hipEvent_t ev[2] = {nullptr, nullptr};
    ~sx_stage_events()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create(sx_ctx *ctx)
    {
        for (hipEvent_t &e : ev) SX_CHECK(hipEventCreate(&e));
        return 0;
    }
};

// device allocations that are released when the scope ends unless someone keeps them: `count` entries rounded up to 256
// bytes plus a 256-byte tail (readable a little beyond the end); bytes_acc, if given, grows by what was allocated
struct sx_dev_scope {
    std::vector<void *> p;
    ~sx_dev_scope()
    {
        for (void *q : p) (void)hipFree(q);
    }
    template <class T> int take(sx_ctx *ctx, T **out, size_t count, size_t *bytes_acc = nullptr)
    {
        void *q = nullptr;
        *out = nullptr;
        const size_t bytes = ((count * sizeof(T) + 255) & ~(size_t)255) + 256;
        if (hipMalloc(&q, bytes) != hipSuccess) {
            (void)hipGetLastError();
            return sx_fail_msg(ctx, SX_E_NOMEM, "device memory of an index or a mapping call");
        }
        p.push_back(q);
        *out = (T *)q;
        if (bytes_acc) *bytes_acc += bytes;
        return 0;
    }
    void drop(void *q)
    {
        const auto it = std::find(p.begin(), p.end(), q);
        if (it == p.end()) return;
        (void)hipFree(q);
        p.erase(it);
    }
    void keep() { p.clear(); }
};
