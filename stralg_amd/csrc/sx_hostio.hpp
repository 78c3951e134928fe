// sx_hostio.hpp -- what the streaming writer (sx_build.hip), the index (sx_index.hip) and the mapper (sx_map.hip) share: the
// context's two pinned staging buffers, the chunked copies through them (sx_hostio.hip), the owner of a call's hipMallocs,
// and the two window loops of the index's compact and sampled forms.
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

// The window loops of sx_occ.hip and sx_locate.hip (they launch nothing themselves).  Down: entries [lo, hi) of entry_bytes
// each, a staging buffer's worth at a time (one at least): fill(lo, hi, d_win) makes a window's, sx_stream_to_sink empties it
template <class Fill>
static int sx_stream_windows(sx_ctx *ctx, int section, uint64_t lo, uint64_t hi, uint64_t entry_bytes, sx_sink_fn sink, void *user, Fill fill)
{
    if (hi <= lo) return 0;
    const uint64_t per = std::min<uint64_t>(std::max<uint64_t>(sx_stage_bytes / entry_bytes, 1), hi - lo);
    sx_dev_scope T;
    uint32_t *d_win;
    SX_TRY(T.take(ctx, &d_win, (size_t)(per * entry_bytes / 4)));
    for (; lo < hi; lo += per) {
        const uint64_t end = hi - lo < per ? hi : lo + per;
        SX_TRY(fill(lo, end, d_win));
        SX_TRY(sx_stream_to_sink(ctx, section, d_win, (size_t)((end - lo) * entry_bytes), sink, user)); // (synchronous: the window is free again)
    }
    return 0;
}

// Up: the rows (row_bytes each) of the N / block_rows + 1 blocks of a host array in windows of as many whole blocks as a
// staging buffer holds beside `extra` rows behind them (one at least); body(d_win, b0, nb, rows): blocks [b0, b0 + nb) are up.
// A body may queue work on ctx->stream that reads the window: the stream is synced before the window is released
template <class Body>
static int sx_upload_windows(sx_ctx *ctx, const void *h_rows, uint64_t N, uint64_t row_bytes, uint32_t block_rows, uint32_t extra, Body body)
{
    const uint64_t nblocks = N / block_rows + 1, fit = sx_stage_bytes / row_bytes;
    const uint64_t per = std::min<uint64_t>(fit > extra + block_rows ? (fit - extra) / block_rows : 1, nblocks);
    sx_dev_scope T;
    uint32_t *d_win;
    SX_TRY(T.take(ctx, &d_win, (size_t)((per * block_rows + extra) * row_bytes / 4)));
    for (uint64_t b0 = 0; b0 < nblocks; b0 += per) {
        const uint32_t nb = (uint32_t)(nblocks - b0 < per ? nblocks - b0 : per);
        const uint64_t row_lo = b0 * block_rows, rows = std::min<uint64_t>((b0 + nb) * block_rows, N) - row_lo + extra;
        if (rows) SX_TRY(sx_upload_staged(ctx, d_win, (const char *)h_rows + row_lo * row_bytes, (size_t)(rows * row_bytes)));
        SX_TRY(body((const uint32_t *)d_win, b0, nb, rows));
    }
    return sx_sync(ctx);
}
