// capi_map.cpp -- mapping: the pinned-block pool, the depth cap, drprg_hip_map_fastx and the host and device batch entries.
#include "capi_ctx.h"
#include "bam.h"
#include "fastx.h"
#include "ingest.h"
#include "pack.h"
#include <algorithm>
#include <atomic>
#include <cstring>

using namespace drprg;

// Page-locked ingest blocks, kept between calls AND between contexts of the process: page-locking costs driver time, in series
// over the threads that ask -- a `drprg predict` that finds a novel variant opens a second context on the updated PRG and maps
// the reads again, and paid for pinning the same blocks a second time while they were kept per context.  (Portable allocations: valid for every
// device.)  The blocks go back to the driver when the last context of the process closes.
struct PinPool {
    std::mutex mu;
    std::vector<std::pair<void*, size_t>> free_, busy_;
    int contexts = 0;
    static PinPool& get()
    {
        static PinPool* p = new PinPool; // (never destroyed: contexts may outlive static destruction order)
        return *p;
    }
    void context_opened()
    {
        std::lock_guard<std::mutex> g(mu);
        ++contexts;
    }
    void context_closed()
    {
        std::vector<std::pair<void*, size_t>> drop;
        {
            std::lock_guard<std::mutex> g(mu);
            if (--contexts > 0) return;
            drop.swap(free_);
        }
        for (auto& b : drop) Mapper::pinned_free(b.first);
    }
    void* take(size_t n)
    {
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < free_.size(); ++i)
                if (free_[i].second == n) {
                    void* p = free_[i].first;
                    free_.erase(free_.begin() + (long)i);
                    busy_.emplace_back(p, n);
                    return p;
                }
        }
        void* p = Mapper::pinned_alloc(n);
        if (p) {
            std::lock_guard<std::mutex> g(mu);
            busy_.emplace_back(p, n);
        }
        return p;
    }
    void give_back(void* p)
    {
        std::lock_guard<std::mutex> g(mu);
        for (size_t i = 0; i < busy_.size(); ++i)
            if (busy_[i].first == p) {
                free_.push_back(busy_[i]);
                busy_.erase(busy_.begin() + (long)i);
                return;
            }
        Mapper::pinned_free(p);
    }
};

void drprg::pin_pool_context_opened() { PinPool::get().context_opened(); }
void drprg::pin_pool_context_closed() { PinPool::get().context_closed(); }

// ---- depth cap -------------------------------------------------------------------------------------------------------------
// T = (max_covg + 1) * genome_size, the bases at which the context stops accepting reads; false: no cap (off, or beyond what a
// 64-bit count of bases can reach)
static bool cap_target(const drprg_hip_ctx* ctx, uint64_t& T)
{
    if (ctx->max_covg >= 0xFFFFFFFFull) return false;
    const unsigned __int128 t = (unsigned __int128)(ctx->max_covg + 1) * ctx->params.genome_size;
    if (t > (unsigned __int128)~0ull) return false;
    T = (uint64_t)t;
    return true;
}

// false: the cap has been reached (by an earlier call, or by a cap set below what is mapped already) -- the n_reads offered are dropped
static bool cap_open(drprg_hip_ctx* ctx, uint64_t n_reads)
{
    uint64_t T;
    if (!ctx->sample.cap_reached && cap_target(ctx, T) && ctx->sample.total_bases >= T) ctx->sample.cap_reached = true;
    if (ctx->sample.cap_reached) ctx->sample.dropped_reads += n_reads;
    return !ctx->sample.cap_reached;
}

// What accepting a batch does to the cap's state.  Worked out before the batch is mapped, committed after the map call has succeeded: a
// call that is refused (bad pointers, a read too long, ...) leaves the context as it was.
struct CapCut {
    bool reached = false;
    uint64_t dropped = 0;
};

static void cap_commit(drprg_hip_ctx* ctx, const CapCut& c, uint64_t n_reads, uint64_t n_bases)
{
    ctx->sample.total_bases += n_bases;
    ctx->sample.accepted_reads += n_reads;
    if (c.reached) {
        ctx->sample.cap_reached = true;
        ctx->sample.dropped_reads += c.dropped;
    }
}

// The host batch cut to the reads the cap accepts: the first i (>= 1; cap_open has said yes) whose bases reach what is still needed (>= 1);
// a packed batch: and to the positions listed for them.  offsets[0] == 0.
static void cap_host_cut(const drprg_hip_ctx* ctx, Mapper::HostBatch& hb, CapCut& c)
{
    uint64_t T;
    if (cap_target(ctx, T) && hb.n_bases() >= T - ctx->sample.total_bases) {
        const uint64_t i = (uint64_t)(std::lower_bound(hb.offsets + 1, hb.offsets + hb.n_reads + 1, T - ctx->sample.total_bases) - hb.offsets);
        c = CapCut { true, hb.n_reads - i };
        hb.n_reads = i;
    }
    if (hb.packed) hb.n_npos = (uint64_t)(std::lower_bound(hb.npos, hb.npos + hb.n_npos, hb.n_bases()) - hb.npos); // (all of them unless the batch was cut)
    if (hb.bam && c.dropped) { // the cut is made on the offsets, before the conversion: the fields of the accepted reads, their non-ACGT codes counted again
        hb.seq_bytes = hb.seq_start[hb.n_reads];
        hb.n_npos = 0;
        for (uint64_t i = 0; i < hb.n_reads; ++i) hb.n_npos += bam::count_non_acgt(hb.bases + hb.seq_start[i], (uint32_t)(hb.offsets[i + 1] - hb.offsets[i]));
    }
}

// The same for a device batch, whose offsets only the device can read: a batch below the cap is accepted as it is, without a look
// at the device; the one that crosses it is cut by covg_cut_kernel (Mapper::find_cut, which first makes the checks the map call itself makes: Mapper::check).
static void cap_device_prefix(const drprg_hip_ctx* ctx, Mapper& m, Mapper::DeviceBatch& b, void* hip_stream, CapCut& c)
{
    uint64_t T;
    if (b.n_reads == 0 || !cap_target(ctx, T) || b.n_bases < T - ctx->sample.total_bases) return;
    const Mapper::CutPoint cut = m.find_cut(b, T - ctx->sample.total_bases, (hipStream_t)hip_stream);
    c = CapCut { true, b.n_reads - cut.n_reads };
    b.n_reads = cut.n_reads; b.n_bases = cut.n_bases; b.n_npos = cut.n_npos;
}

// ---- drprg_hip_map_fastx ----------------------------------------------------------------------------------------------------
// What one call shares between its steps.  filter: the read filter (drprg_hip_set_read_filter) as it stood when the call began.  Every block goes through Mapper::map_host_filtered on
// the device that takes it, and everything behind it -- the counters, the depth cap's running total, the resident set -- sees the kept reads
// alone.  Not set: nothing differs from a build without it (no quality byte is parsed or copied, no launch, no wait).
// ordered: under a depth cap, or drprg_hip_set_ordered_ingest (the same hand-over without a cap: nothing is ever cut), the blocks come in file
// order, one at a time, and are counted where they are handed to the devices, round robin from rr.  Otherwise, over several devices
// (drprg_hip_open_multi), the reads shard by block (submit_to_idle_device) and the parser threads that carry the blocks are the submitters.
namespace {
struct FastxPass {
    drprg_hip_ctx* ctx;
    const Mapper::ReadFilter filter;
    const bool ordered;
    const std::vector<Mapper*> devs;
    std::vector<std::mutex> dev_mu; // one submitter per device at a time
    std::atomic<size_t> next_dev { 0 };
    size_t rr = 0;
    std::atomic<uint64_t> kept_reads { 0 }, kept_bases { 0 }; // what the filter kept of the blocks handed over in no order
    FastxPass(drprg_hip_ctx* c, bool in_order) : ctx(c), filter(c->read_filter), ordered(in_order), devs(mappers_of(c)), dev_mu(devs.size()) {}
};
} // namespace

static Mapper::HostBatch host_batch(const PinnedBatch& b)
{
    return Mapper::HostBatch { b.bases, b.offsets, b.n_reads, b.packed, b.npos, b.n_npos, b.bam, b.seq_start, b.reverse, b.seq_bytes, b.qual, b.qual_bias };
}

// A block through the filter on `dev`; what it counted goes to the context's counts (the submitters are one per device: filter_mu).
static Mapper::FilterOutcome map_filtered(drprg_hip_ctx* ctx, const Mapper::ReadFilter& filter, Mapper& dev, const Mapper::HostBatch& hb, uint64_t cap_need)
{
    Mapper::FilterOutcome o;
    dev.map_host_filtered(hb, filter, cap_need, o);
    std::lock_guard<std::mutex> g(ctx->filter_mu);
    ctx->sample.filter_counts += o;
    return o;
}

// One block, on this mapper, under the context's cap.  The block that crosses the cap reaches its device cut to the accepted reads (so a
// device that keeps its blocks resident keeps exactly those): filtered, the cap cuts on the kept reads' running total and the device finds the
// read (Mapper::map_host_filtered); unfiltered, the cut is made here.  The cap's state is committed once the map call has succeeded.
// wait: the caller reuses the block's buffers at once, so the mapper is done with them on return.  Returns whether the ingest goes on.
// count: read statistics, when they are set (the blocks of drprg_hip_map_fastx: the host entries carry no qualities and are not counted).
static bool map_block_capped(drprg_hip_ctx* ctx, const Mapper::ReadFilter& filter, Mapper& dev, Mapper::HostBatch hb, bool wait, bool count = false)
{
    if (filter.any()) {
        uint64_t T = 0;
        const Mapper::FilterOutcome o = map_filtered(ctx, filter, dev, hb, cap_target(ctx, T) ? T - ctx->sample.total_bases : 0);
        if (wait) dev.sync();
        cap_commit(ctx, CapCut { o.cut, o.cut_dropped }, o.mapped_reads, o.mapped_bases);
    } else {
        CapCut c;
        Mapper::HostBatch whole = hb;
        cap_host_cut(ctx, hb, c);
        if (count && filter.read_stats) { // under a cap the two snapshots differ: raw takes the block as the file held it, prepared what the cap accepts
            uint64_t T = 0;
            hb.stats_mode = whole.stats_mode = (uint8_t)filter.read_stats;
            hb.stats_which = cap_target(ctx, T) ? 3 : 1;
            if (c.dropped) {
                whole.stats_which = 1;
                dev.count_host_block(whole);
                hb.stats_which = 2;
            }
        }
        if (wait) dev.map_host(hb);
        else dev.map_host_async(hb); // (the copy of a block overlaps the kernels of the block before it)
        cap_commit(ctx, c, hb.n_reads, hb.n_bases());
    }
    return !ctx->sample.cap_reached;
}

// A block handed over in no particular order: nothing is cut, and the cap's totals are counted once, after the ingest (count_ingest).
static void map_block_unordered(FastxPass& p, Mapper& dev, const Mapper::HostBatch& hb)
{
    if (!p.filter.any()) {
        Mapper::HostBatch counted = hb;
        counted.stats_mode = (uint8_t)p.filter.read_stats; // (nothing is prepared and nothing is cut: the raw snapshot stands for both)
        counted.stats_which = p.filter.read_stats ? 1 : 0;
        return dev.map_host_async(counted);
    }
    const Mapper::FilterOutcome o = map_filtered(p.ctx, p.filter, dev, hb, 0);
    p.kept_reads += o.mapped_reads;
    p.kept_bases += o.mapped_bases;
}

// Several devices, no order: the first idle one, round robin from the one after the last choice; all busy: wait for that choice.
static void submit_to_idle_device(FastxPass& p, const PinnedBatch& b)
{
    const size_t ndev = p.devs.size(), first = p.next_dev.fetch_add(1) % ndev;
    for (size_t i = 0; i < ndev; ++i) {
        const size_t d = (first + i) % ndev;
        std::unique_lock<std::mutex> l(p.dev_mu[d], std::try_to_lock);
        if (!l.owns_lock()) continue;
        return map_block_unordered(p, *p.devs[d], host_batch(b));
    }
    std::lock_guard<std::mutex> l(p.dev_mu[first]);
    map_block_unordered(p, *p.devs[first], host_batch(b));
}

// The multi-threaded ingest into pinned blocks (ingest.cpp) and where its blocks go.
static IngestHooks fastx_hooks(FastxPass& p)
{
    IngestHooks hooks;
    hooks.packed = p.ctx->packed_input;
    hooks.bam_native = true; // a BAM file's reads travel in their 4-bit form and are converted on the device (bam_pack.hip), whatever `packed` says
    hooks.want_qual = p.filter.wants_qual(); // (for the filter's threshold, --trim-qual, --mask-qual or --qc-json; fixed crops alone carry none)
    if (p.filter.read_stats == 1) hooks.qual_flag = "--qc-json"; // (any other quality setting is named first)
    if (p.filter.use_qual()) hooks.qual_flag = "--min-read-qual";
    if (p.filter.mask_qual) hooks.qual_flag = "--mask-qual";
    if (p.filter.trim_qual_milli) hooks.qual_flag = "--trim-qual"; // (trimming comes first, then the mask: the first to miss them is named)
    // page-locked ingest blocks are kept by the process between calls and contexts (PinPool)
    hooks.alloc = [](size_t n) -> void* { return PinPool::get().take(n); };
    hooks.release = [](void* q) { PinPool::get().give_back(q); };
    if (p.devs.size() == 1) hooks.submit = [&p](const PinnedBatch& b) { map_block_unordered(p, *p.devs[0], host_batch(b)); }; // (the ingest serialises the calls)
    else {
        hooks.concurrent_submit = true;
        hooks.submit = [&p](const PinnedBatch& b) { submit_to_idle_device(p, b); };
    }
    // (once a block has crossed the cap nothing after it is copied anywhere and the ingest takes no new piece of the file)
    if (p.ordered)
        hooks.submit_in_order = [&p](const PinnedBatch& b) -> bool {
            if (b.offsets[0] != 0) throw Error(DRPRG_EINVAL, "offsets[0] must be 0");
            return map_block_capped(p.ctx, p.filter, *p.devs[p.rr++ % p.devs.size()], host_batch(b), false, true);
        };
    return hooks;
}

// What the ingest says once the file is through.  Ordered: the accepted reads were counted block by block.  Unordered: all of them here.
static void count_ingest(FastxPass& p, const IngestStats& st)
{
    SampleState& s = p.ctx->sample;
    s.bam_records += st.bam_records; s.bam_skipped += st.bam_skipped; s.bam_reversed += st.bam_reversed;
    if (p.ordered) s.dropped_reads += st.discarded_reads;
    else {
        s.total_bases += p.filter.any() ? p.kept_bases.load() : st.bases;
        s.accepted_reads += p.filter.any() ? p.kept_reads.load() : st.reads;
        if (st.batches > 1) s.fastx_unordered = true;
    }
}

// What the parallel ingest hands back (DRPRG_EAGAIN_SERIAL: multi-line FASTQ): the serial reader, batch by batch on the first device, each
// batch waited for because its buffers go with the next read.
static void map_fastx_serial(FastxPass& p, const char* reads_path)
{
    const Mapper::ReadFilter& filter = p.filter;
    FastxReader rd(reads_path);
    ReadBatch batch;
    while (rd.next_batch(batch, 8u << 20, 1ull << 30, false, filter.wants_qual())) {
        if (!batch.n_reads()) continue;
        Mapper::HostBatch hb { batch.bases.data(), batch.offsets.data(), batch.n_reads() };
        if (filter.any()) {
            if (filter.trim_qual_milli && batch.qual.size() != batch.bases.size())
                throw Error(DRPRG_EINVAL, "--trim-qual: a FASTA record has no base qualities; a read is never trimmed by a quality it does not have");
            if (filter.mask_qual && batch.qual.size() != batch.bases.size())
                throw Error(DRPRG_EINVAL, "--mask-qual: a FASTA record has no base qualities; a base is never masked by a quality it does not have");
            if (filter.use_qual() && batch.qual.size() != batch.bases.size())
                throw Error(DRPRG_EINVAL, "--min-read-qual: a FASTA record has no base qualities; a read is never kept or dropped by a quality threshold it cannot be held against");
        }
        if (filter.read_stats == 1 && batch.qual.size() != batch.bases.size())
            throw Error(DRPRG_EINVAL, "--qc-json: a FASTA record has no base qualities; the read statistics report them (--qc-no-qual reports without them)");
        if (filter.wants_qual()) hb.qual = batch.qual.data();
        if (filter.any() || filter.read_stats) hb.qual_bias = 33;
        if (!map_block_capped(p.ctx, filter, *p.devs[0], hb, true, true)) break;
    }
}

extern "C" {

int drprg_hip_map_fastx(drprg_hip_ctx* ctx, const char* reads_path)
{
    API_BEGIN(ctx)
    if (!reads_path) throw Error(DRPRG_EINVAL, "null reads path");
    need_mapper(ctx);
    if (!cap_open(ctx, 0)) return DRPRG_OK; // the depth cap was reached before this call: the file is not opened
    ctx->sample.host_coverage_valid = false;
    ctx->sample.mapped_paths.push_back(reads_path);
    uint64_t T = 0;
    FastxPass pass(ctx, cap_target(ctx, T) || ctx->ordered_ingest);
    if (pass.filter.read_stats && (pass.filter.any() || cap_target(ctx, T))) ctx->sample.stats_prepared = true; // (else the raw snapshot stands for both)
    const IngestHooks hooks = fastx_hooks(pass);
    try {
        count_ingest(pass, ingest_fastx(reads_path, ctx->threads, hooks));
        // the coverage vectors of the other devices are summed into device 0 ON THE DEVICE (reduce_devices); unsigned sums commute, so the
        // result does not depend on which device mapped which block
        for (Mapper* m : mappers_of(ctx)) m->sync();
        reduce_devices(ctx);
    } catch (const Error& e) {
        if (e.code != DRPRG_EAGAIN_SERIAL) throw; // (a failed multi-device pass leaves partial vectors on the devices: reset before reuse)
        map_fastx_serial(pass, reads_path);
    }
    if (pass.filter.read_stats) // what the statistics kernels refused, once per pass (a block behind a prep stage has said so itself)
        for (Mapper* m : mappers_of(ctx)) m->check_read_stats();
    API_END(ctx)
}

int drprg_hip_set_max_covg(drprg_hip_ctx* ctx, uint64_t max_covg)
{
    if (!ctx) return DRPRG_EINVAL;
    ctx->max_covg = max_covg; // (>= 2^32 - 1: off; what is mapped already counts -- cap_open looks at the running total)
    return DRPRG_OK;
}

int drprg_hip_max_covg_info(drprg_hip_ctx* ctx, uint64_t out[4])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    for (Mapper* m : mappers_of(ctx)) m->sync();
    (void)cap_open(ctx, 0);
    const SampleState& s = ctx->sample;
    out[0] = s.cap_reached ? 1 : 0; out[1] = s.accepted_reads; out[2] = s.total_bases; out[3] = s.dropped_reads;
    API_END(ctx)
}

int drprg_hip_set_threads(drprg_hip_ctx* ctx, int threads)
{
    if (!ctx) return DRPRG_EINVAL;
    ctx->threads = threads > 0 ? threads : 1;
    return DRPRG_OK;
}

// ---- host and device batches -------------------------------------------------------------------------------------------------
// These entry points carry no qualities: while a filter is set they refuse, rather than map unfiltered reads without saying so.
static void refuse_unfiltered(const drprg_hip_ctx* ctx, const char* entry)
{
    if (ctx->pair.on())
        throw Error(DRPRG_EINVAL, std::string(entry) + ": a mate-overlap setting is on (drprg_hip_set_pair_overlap) and the sides are numbered in "
                                                      "drprg_hip_map_fastx; this entry would map reads that have no mate (clear it with "
                                                      "drprg_hip_set_pair_overlap(ctx, 0, 0, 0))");
    if (ctx->read_filter.decoy())
        throw Error(DRPRG_EINVAL, std::string(entry) + ": a decoy set is loaded (drprg_hip_set_decoy) and the screen runs in drprg_hip_map_fastx; this entry "
                                                      "would map the reads unscreened (clear it with drprg_hip_set_decoy(ctx, NULL, 0, 0, 0, 0))");
    if (ctx->read_filter.any_adapters())
        throw Error(DRPRG_EINVAL, std::string(entry) + ": adapters are set (drprg_hip_set_adapters) and adapter trimming runs in drprg_hip_map_fastx; this entry "
                                                      "would map the reads with their adapters (clear them with drprg_hip_set_adapters(ctx, NULL, 0, 0, 0))");
    if (ctx->read_filter.poly())
        throw Error(DRPRG_EINVAL, std::string(entry) + ": poly-tail trimming is set (drprg_hip_set_poly_trim) and runs in drprg_hip_map_fastx; this entry "
                                                      "would map the reads with their tails (clear it with drprg_hip_set_poly_trim(ctx, NULL, 0))");
    if (ctx->read_filter.min_complexity)
        throw Error(DRPRG_EINVAL, std::string(entry) + ": a complexity threshold is set (drprg_hip_set_min_complexity) and the test runs in drprg_hip_map_fastx; "
                                                      "this entry would map the reads unjudged (clear it with drprg_hip_set_min_complexity(ctx, 0))");
    if (ctx->read_filter.trims())
        throw Error(DRPRG_EINVAL, std::string(entry) + ": read trimming is set (drprg_hip_set_read_trim) and this entry carries no qualities; trimming "
                                                      "runs in drprg_hip_map_fastx (clear it with drprg_hip_set_read_trim(ctx, 0, 0, 0, 0))");
    if (ctx->read_filter.mask_qual)
        throw Error(DRPRG_EINVAL, std::string(entry) + ": a base mask is set (drprg_hip_set_base_mask) and this entry carries no qualities; masking runs in "
                                                      "drprg_hip_map_fastx (clear it with drprg_hip_set_base_mask(ctx, 0))");
    if (ctx->read_filter.read_stats == 1)
        throw Error(DRPRG_EINVAL, std::string(entry) + ": read statistics with qualities are set (drprg_hip_set_read_stats) and this entry carries no qualities; "
                                                      "the statistics are taken in drprg_hip_map_fastx (clear them with drprg_hip_set_read_stats(ctx, 0))");
    if (ctx->read_filter.any())
        throw Error(DRPRG_EINVAL, std::string(entry) + ": a read filter is set (drprg_hip_set_read_filter) and this entry carries no qualities; the filter "
                                                      "runs in drprg_hip_map_fastx (clear it with drprg_hip_set_read_filter(ctx, 0, 0, 0))");
}

// A host batch in either form: cut at the depth cap (the offsets are here), mapped and waited for, counted -- the capped-block step of
// drprg_hip_map_fastx, with no filter set.  The entry points have refused null buffers.
static void map_host_batch(drprg_hip_ctx* ctx, const Mapper::HostBatch& hb)
{
    Mapper& m = need_mapper(ctx);
    refuse_unfiltered(ctx, "drprg_hip_map_host*");
    if (hb.n_reads && cap_open(ctx, hb.n_reads)) {
        if (hb.offsets[0] != 0) throw Error(DRPRG_EINVAL, "offsets[0] must be 0");
        (void)map_block_capped(ctx, ctx->read_filter, m, hb, true);
    }
    ctx->sample.host_coverage_valid = false;
}

int drprg_hip_map_host(drprg_hip_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n_reads)
{
    API_BEGIN(ctx)
    if (n_reads && (!bases || !offsets)) throw Error(DRPRG_EINVAL, "null buffer");
    map_host_batch(ctx, Mapper::HostBatch { bases, offsets, n_reads });
    API_END(ctx)
}

// ---- 2-bit packed reads (SURVEY.md section 8f NEXT-4) ----
int drprg_hip_set_input_format(drprg_hip_ctx* ctx, int packed)
{
    if (!ctx) return DRPRG_EINVAL;
    ctx->packed_input = packed != 0;
    return DRPRG_OK;
}

int drprg_hip_pack_reads(const uint8_t* bases, uint64_t n_bases, uint32_t* words, uint64_t* npos, uint64_t npos_cap, uint64_t* n_npos)
{
    if ((n_bases && (!bases || !words)) || !n_npos) return DRPRG_EINVAL;
    try {
        // (pack_append works on 64-bit words and writes one word past the last base: through a buffer of its own)
        std::vector<uint64_t> w64(n_bases / 32 + 2, 0);
        std::vector<uint64_t> np;
        uint64_t n = 0;
        if (n_bases) pack_append(w64.data(), n, reinterpret_cast<const char*>(bases), n_bases, np);
        std::memcpy(words, w64.data(), (n_bases + 15) / 16 * sizeof(uint32_t));
        *n_npos = np.size();
        if (np.size() > npos_cap) return DRPRG_EOVERFLOW;
        if (!np.empty()) {
            if (!npos) return DRPRG_EINVAL;
            std::memcpy(npos, np.data(), np.size() * sizeof(uint64_t));
        }
    } catch (const std::bad_alloc&) {
        return DRPRG_ENOMEM;
    }
    return DRPRG_OK;
}

int drprg_hip_map_host_packed(drprg_hip_ctx* ctx, const uint32_t* words, const uint64_t* offsets, uint64_t n_reads, const uint64_t* npos, uint64_t n_npos)
{
    API_BEGIN(ctx)
    if (n_reads && (!words || !offsets)) throw Error(DRPRG_EINVAL, "null buffer");
    if (n_npos && !npos) throw Error(DRPRG_EINVAL, "n_npos > 0 without the positions");
    map_host_batch(ctx, Mapper::HostBatch { reinterpret_cast<const uint8_t*>(words), offsets, n_reads, true, npos, n_npos });
    API_END(ctx)
}

// Behind the four device entry points: a batch that crosses the depth cap is cut to the accepted reads, then mapped, then counted.
static int map_device_batch(drprg_hip_ctx* ctx, Mapper::DeviceBatch b, void* d_covg, void* d_prg_reads, void* hip_stream, bool deferred)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    refuse_unfiltered(ctx, "drprg_hip_map_device*");
    if (b.n_reads == 0 || cap_open(ctx, b.n_reads)) { // (an empty batch still goes through the mapper's argument checks)
        CapCut c;
        cap_device_prefix(ctx, m, b, hip_stream, c);
        m.map(b, (uint32_t*)d_covg, (uint32_t*)d_prg_reads, (hipStream_t)hip_stream, deferred);
        cap_commit(ctx, c, b.n_reads, b.n_bases);
    }
    ctx->sample.host_coverage_valid = false;
    API_END(ctx)
}

static Mapper::DeviceBatch device_batch(const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, bool packed = false,
    const void* d_npos = nullptr, uint64_t n_npos = 0)
{
    return Mapper::DeviceBatch { (const uint8_t*)d_bases, (const uint64_t*)d_offsets, n_reads, n_bases, packed, (const uint64_t*)d_npos, n_npos };
}

int drprg_hip_map_device_packed(drprg_hip_ctx* ctx, const void* d_words, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void* d_npos,
    uint64_t n_npos, void* d_covg, void* d_prg_reads, void* hip_stream)
{
    return map_device_batch(ctx, device_batch(d_words, d_offsets, n_reads, n_bases, true, d_npos, n_npos), d_covg, d_prg_reads, hip_stream, false);
}

int drprg_hip_map_device_packed_async(drprg_hip_ctx* ctx, const void* d_words, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void* d_npos,
    uint64_t n_npos, void* d_covg, void* d_prg_reads, void* hip_stream)
{
    return map_device_batch(ctx, device_batch(d_words, d_offsets, n_reads, n_bases, true, d_npos, n_npos), d_covg, d_prg_reads, hip_stream, true);
}

int drprg_hip_pack_device(drprg_hip_ctx* ctx, const void* d_bases, uint64_t n_bases, void* d_words, void* d_npos, uint64_t npos_cap, uint64_t* n_npos,
    void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!n_npos) throw Error(DRPRG_EINVAL, "null n_npos");
    *n_npos = m.pack_on_device((const uint8_t*)d_bases, n_bases, (uint32_t*)d_words, (uint64_t*)d_npos, npos_cap, (hipStream_t)hip_stream);
    if (*n_npos > npos_cap) throw Error(DRPRG_EOVERFLOW, "more non-ACGT bases than the position buffer holds");
    API_END(ctx)
}

int drprg_hip_pack_device_bam(drprg_hip_ctx* ctx, const void* d_seq, const void* d_seq_start, const void* d_offsets, const void* d_reverse, uint64_t n_reads,
    uint64_t n_bases, void* d_words, void* d_npos, uint64_t npos_cap, uint64_t* n_npos, void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!n_npos) throw Error(DRPRG_EINVAL, "null n_npos");
    *n_npos = m.pack_bam_on_device((const uint8_t*)d_seq, (const uint64_t*)d_seq_start, (const uint64_t*)d_offsets, (const uint8_t*)d_reverse, n_reads, n_bases,
        (uint32_t*)d_words, (uint64_t*)d_npos, npos_cap, (hipStream_t)hip_stream);
    if (*n_npos > npos_cap) throw Error(DRPRG_EOVERFLOW, "more non-ACGT bases than the position buffer holds");
    API_END(ctx)
}

int drprg_hip_bam_info(drprg_hip_ctx* ctx, uint64_t out[4])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    out[0] = ctx->sample.bam_records; out[1] = ctx->sample.bam_skipped; out[2] = ctx->sample.bam_reversed; out[3] = 0;
    for (Mapper* m : mappers_of(ctx)) out[3] += m->bam_blocks();
    API_END(ctx)
}

int drprg_hip_map_device(drprg_hip_ctx* ctx, const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
    void* d_covg, void* d_prg_reads, void* hip_stream)
{
    return map_device_batch(ctx, device_batch(d_bases, d_offsets, n_reads, n_bases), d_covg, d_prg_reads, hip_stream, false);
}

int drprg_hip_map_device_async(drprg_hip_ctx* ctx, const void* d_bases, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
    void* d_covg, void* d_prg_reads, void* hip_stream)
{
    return map_device_batch(ctx, device_batch(d_bases, d_offsets, n_reads, n_bases), d_covg, d_prg_reads, hip_stream, true);
}

int drprg_hip_set_ordered_ingest(drprg_hip_ctx* ctx, int on)
{
    if (!ctx) return DRPRG_EINVAL;
    ctx->ordered_ingest = on != 0;
    return DRPRG_OK;
}

} // extern "C"
