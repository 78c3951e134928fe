// sx_hostio.hip -- the pinned staging buffers of a context, the chunked copies through them (sx_hostio.hpp), sx_download.
#include "sx_hostio.hpp"

int sx_stage_ensure(sx_ctx *ctx)
{
    for (char *&b : ctx->h_stage)
        if (!b && hipHostMalloc((void **)&b, sx_stage_bytes, hipHostMallocDefault) != hipSuccess) {
            b = nullptr;
            (void)hipGetLastError();
            return sx_fail_msg(ctx, SX_E_NOMEM, "pinned staging buffers");
        }
    return 0;
}

int sx_stream_to_sink(sx_ctx *ctx, int section, const void *d_src, size_t bytes, sx_sink_fn sink, void *user)
{
    SX_TRY(sx_stage_ensure(ctx));
    const char *src = (const char *)d_src;
    size_t off = 0, pending = bytes < sx_stage_bytes ? bytes : sx_stage_bytes;
    int cur = 0;
    if (pending) SX_CHECK(hipMemcpyAsync(ctx->h_stage[0], src, pending, hipMemcpyDeviceToHost, ctx->stream));
    while (pending) {
        SX_CHECK(hipStreamSynchronize(ctx->stream));
        const size_t have = pending;
        off += have;
        const size_t next = bytes - off < sx_stage_bytes ? bytes - off : sx_stage_bytes;
        if (next) SX_CHECK(hipMemcpyAsync(ctx->h_stage[cur ^ 1], src + off, next, hipMemcpyDeviceToHost, ctx->stream));
        if (sink(user, section, ctx->h_stage[cur], have) != 0) {
            (void)hipStreamSynchronize(ctx->stream);
            return sx_fail_msg(ctx, SX_E_ARG, "the sink refused a chunk");
        }
        pending = next;
        cur ^= 1;
    }
    return 0;
}

int sx_download(sx_ctx *ctx, void *h_dst, const void *d_src, size_t bytes)
{
    if (!ctx || (bytes && (!h_dst || !d_src))) return SX_E_ARG;
    SX_CHECK(hipSetDevice(ctx->device));
    if (bytes) SX_CHECK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return sx_sync(ctx);
}

int sx_upload_staged(sx_ctx *ctx, void *d_dst, const void *h_src, size_t bytes)
{
    if (!bytes) return 0;
    SX_TRY(sx_stage_ensure(ctx));
    sx_stage_events E;
    SX_TRY(E.create(ctx));
    bool ok = true;
    for (size_t off = 0, k = 0; ok && off < bytes; ++k) {
        const size_t n = bytes - off < sx_stage_bytes ? bytes - off : sx_stage_bytes, b = k & 1;
        ok = k < 2 || hipEventSynchronize(E.ev[b]) == hipSuccess; // (the copy that last used this buffer is done)
        if (!ok) break;
        memcpy(ctx->h_stage[b], (const char *)h_src + off, n);
        ok = hipMemcpyAsync((char *)d_dst + off, ctx->h_stage[b], n, hipMemcpyHostToDevice, ctx->stream) == hipSuccess &&
             hipEventRecord(E.ev[b], ctx->stream) == hipSuccess;
        off += n;
    }
    // (whatever happened: no copy out of the staging buffers is in flight when the call returns)
    ok = hipStreamSynchronize(ctx->stream) == hipSuccess && ok;
    return ok ? 0 : sx_fail_msg(ctx, SX_E_INTERNAL, "staged upload");
}
