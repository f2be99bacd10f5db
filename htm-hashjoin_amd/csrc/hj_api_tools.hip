// hj_api_tools.hip -- the C ABI's tools around the joins: the streaming Zipf generator and the shard helpers of the
// multi-GPU host. Host-side glue only.
#include "hj_host.h"

#include <new>
#include <vector>

using namespace hjapi;

void hjapi::zipf_release(hj_ctx* c)
{
    delete c->zipf.rng;
    if (c->zipf.lut) hipFree(c->zipf.lut);
    if (c->zipf.alphabet) hipFree(c->zipf.alphabet);
    for (int i = 0; i < 2; ++i) {
        if (c->zipf.rawHost[i]) hipHostFree(c->zipf.rawHost[i]);
        if (c->zipf.rawDev[i]) hipFree(c->zipf.rawDev[i]);
        if (c->zipf.done[i]) hipEventDestroy(c->zipf.done[i]);
    }
    c->zipf = {};
}

extern "C" {

// ---- streaming Zipf generator ---------------------------------------------------
int hj_zipf_open(hj_ctx* c, uint64_t alphabetSize, double theta, unsigned seed)
{
    if (!c) return HJ_ERR_INVALID;
    if (alphabetSize == 0 || alphabetSize > 0xFFFFFFFFull || !(theta >= 0.0)) return fail(c, HJ_ERR_INVALID, "hj_zipf_open: alphabet in [1, 2^32), theta >= 0");
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    zipf_release(c);
    c->zipf.rng = new (std::nothrow) hjhost::GlibcRand(seed);
    if (!c->zipf.rng) return HJ_ERR_OOM;
    std::vector<uint32_t> alphabet;
    std::vector<double> lut;
    hjhost::zipf_tables(*c->zipf.rng, (uint32_t)alphabetSize, theta, alphabet, lut);       // consumes alphabetSize - 1 draws
    HJ_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->zipf.lut), alphabetSize * sizeof(double)));
    HJ_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->zipf.alphabet), alphabetSize * sizeof(uint32_t)));
    HJ_HIP(c, hipMemcpy(c->zipf.lut, lut.data(), alphabetSize * sizeof(double), hipMemcpyHostToDevice));
    HJ_HIP(c, hipMemcpy(c->zipf.alphabet, alphabet.data(), alphabetSize * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->zipf.alphabetSize = (uint32_t)alphabetSize;
    for (int i = 0; i < 2; ++i) HJ_HIP(c, hipEventCreateWithFlags(&c->zipf.done[i], hipEventDisableTiming));
    return HJ_OK;
}

int hj_zipf_next_dev(hj_ctx* c, uint64_t n, uint64_t* dOut)
{
    HJ_ENTER(c, dOut || !n);
    if (!c->zipf.rng) return fail(c, HJ_ERR_STATE, "hj_zipf_next_dev: hj_zipf_open() first");
    HJ_HIP(c, hipSetDevice(c->device));
    // pieces of at most 2^26 draws through two pinned buffers: the host draws piece k + 1 of the serial rand() stream
    // while the device still copies and searches piece k
    const uint64_t piece = 1ull << 26;
    if (c->zipf.rawCap == 0) {
        for (int i = 0; i < 2; ++i) {
            HJ_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->zipf.rawHost[i]), piece * sizeof(int)));
            HJ_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->zipf.rawDev[i]), piece * sizeof(int)));
        }
        c->zipf.rawCap = piece;
    }
    for (uint64_t off = 0; off < n; off += piece) {
        const uint64_t m = n - off < piece ? n - off : piece;
        const int b = c->zipf.flip;
        c->zipf.flip ^= 1;
        HJ_HIP(c, hipEventSynchronize(c->zipf.done[b]));          // the previous use of this buffer pair has been consumed
        int* h = c->zipf.rawHost[b];
        for (uint64_t i = 0; i < m; ++i) h[i] = c->zipf.rng->next();
        HJ_HIP(c, hipMemcpyAsync(c->zipf.rawDev[b], h, m * sizeof(int), hipMemcpyHostToDevice, c->stream));
        launch_zipf_lookup(c->zipf.rawDev[b], m, c->zipf.lut, c->zipf.alphabet, c->zipf.alphabetSize, dOut + off, c->stream);
        HJ_HIP(c, hipGetLastError());
        HJ_HIP(c, hipEventRecord(c->zipf.done[b], c->stream));
    }
    return HJ_OK;
}

int hj_zipf_close(hj_ctx* c)
{
    if (!c) return HJ_ERR_INVALID;
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    zipf_release(c);
    return HJ_OK;
}

// ---- shard helpers -----------------------------------------------------------
int hj_set_shard_check(hj_ctx* c, uint32_t nShards, uint32_t mode, uint32_t shardId)
{
    if (!c) return HJ_ERR_INVALID;
    if (nShards == 0) { c->sc = ShardCheck{0, 0, 0, 0}; return HJ_OK; }
    if (!is_pow2(nShards) || nShards > 64 || shardId >= nShards || (mode & 0xFFu) > 31 || (mode >> 9) != 0)
        return fail(c, HJ_ERR_INVALID, "hj_set_shard_check: nShards a power of two <= 64, shardId < nShards, mode as for hj_shard_histogram_dev");
    c->sc = ShardCheck{nShards - 1, mode & 0xFFu, (mode >> 8) & 1u, shardId};
    return HJ_OK;
}

static int shard_check(hj_ctx* c, const char* who, uint64_t n, uint32_t nShards, uint32_t mode)
{
    if (!is_pow2(nShards) || nShards > 64) return fail(c, HJ_ERR_INVALID, who);
    if ((mode & 0xFFu) > 31 || (mode >> 9) != 0)
        return fail(c, HJ_ERR_INVALID, "shard helpers: mode = digit position (0..31), optionally | HJ_SHARD_ONE_BASED");
    if (n >= 0xFFFFFFFFull) return fail(c, HJ_ERR_INVALID, "shard helpers: n must be < 2^32");
    return HJ_OK;
}

int hj_shard_histogram_dev(hj_ctx* c, const uint64_t* dIn, uint64_t n, uint32_t nShards, uint32_t mode,
                           uint64_t* dCounts)
{
    HJ_ENTER(c, (dIn || !n) && dCounts);
    int rc = shard_check(c, "hj_shard_histogram_dev: nShards must be a power of two <= 64", n, nShards, mode);
    if (rc) return rc;
    HJ_HIP(c, hipSetDevice(c->device));
    // reuse the slot of the same input, else the least recently used one
    hj_ctx::ShardPlan* slot = &c->shards.plan[0];
    for (auto& sp : c->shards.plan) if (sp.in == dIn && sp.n == n) { slot = &sp; break; } else if (sp.stamp < slot->stamp) slot = &sp;
    DevBuf& work = c->buf[B_SHARD0 + (slot - c->shards.plan)];
    if ((rc = work.reserve(c, shard_work_bytes(n, nShards)))) return rc;
    slot->in = dIn; slot->n = n; slot->nShards = nShards; slot->mode = mode; slot->stamp = ++c->shards.stamp;
    HJ_HIP(c, launch_shard_hist(dIn, n, nShards, mode, work.p, reinterpret_cast<unsigned long long*>(dCounts), c->stream));
    return HJ_OK;
}

int hj_shard_scatter_dev(hj_ctx* c, const uint64_t* dIn, uint64_t n, uint32_t nShards, uint32_t mode,
                         const uint64_t* dCounts, uint32_t* dOutKeys)
{
    HJ_ENTER(c, (dIn || !n) && dCounts && (dOutKeys || !n));
    int rc = shard_check(c, "hj_shard_scatter_dev: nShards must be a power of two <= 64", n, nShards, mode);
    if (rc) return rc;
    hj_ctx::ShardPlan* slot = nullptr;
    for (auto& sp : c->shards.plan) if (sp.in == dIn && sp.n == n && sp.nShards == nShards && sp.mode == mode && c->buf[B_SHARD0 + (&sp - c->shards.plan)].p) slot = &sp;
    if (!slot) return fail(c, HJ_ERR_STATE, "hj_shard_scatter_dev: call hj_shard_histogram_dev on this input (same nShards and mode) first");
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, launch_shard_scatter_ordered(dIn, n, nShards, mode, c->buf[B_SHARD0 + (slot - c->shards.plan)].p, dOutKeys, c->stream));
    slot->in = nullptr;   // consumed
    return HJ_OK;
}

}  // extern "C"
