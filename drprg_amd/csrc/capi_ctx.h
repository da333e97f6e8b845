// capi_ctx.h -- what the translation units behind include/drprg_hip.h (capi*.cpp) share: the context and the helpers that more
// than one of them calls.  Internal: not installed, and nothing declared here is exported from the library.
#pragma once
#include "../../include/drprg_hip.h"
#include "denovo.h"
#include "genotype.h"
#include "mapper.h"
#include "rccl_dyn.h"
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#pragma GCC visibility push(hidden)

namespace drprg {
// the process-wide pool of page-locked ingest blocks counts the open contexts (capi_map.cpp PinPool)
void pin_pool_context_opened();
void pin_pool_context_closed();

// the last drprg_hip_subsample / drprg_hip_dedup: whether there was one, the reads of the sample before it, their keep flags (empty: none dropped)
struct Selection {
    bool done = false;
    uint64_t reads_before = 0;
    std::vector<uint8_t> flags;
    uint64_t counts[4] = { 0, 0, 0, 0 }; // the call's four outputs: reads and bases before, reads and bases kept
};

// What the context knows of the sample it is mapping: all of it, and nothing else, goes back to this with drprg_hip_reset.
struct SampleState {
    // host copy of the coverage (drprg_hip_set_coverage, drprg_hip_load_coverage, or downloaded lazily: sync_host_coverage)
    std::vector<uint32_t> covg, prg_reads;
    bool host_coverage_valid = false; // cleared by everything that maps or reduces
    // The depth cap's running state (capi_map.cpp cap_open / cap_commit; the rule is in include/drprg_hip.h), total_bases the running total B.
    // Written too by set_coverage and load_coverage, drprg_hip_map_resident (the other context's), drprg_hip_subsample and drprg_hip_dedup (the kept reads').
    uint64_t total_bases = 0;
    bool cap_reached = false;
    uint64_t accepted_reads = 0, dropped_reads = 0;
    bool bases_without_reads = false; // total_bases holds bases that came with a coverage vector (set_coverage, load_coverage): accepted_reads does not stand for them
    uint64_t bam_records = 0, bam_skipped = 0, bam_reversed = 0; // drprg_hip_map_fastx, of the BAM files it mapped (drprg_hip_bam_info)
    // the files drprg_hip_map_fastx has mapped (the resident reads stand for a file only if they are that file's and nothing else's:
    // reads_resident; drprg_hip_keep_reads and drprg_hip_map_resident write it too); and whether it handed more than one block over in no
    // particular order (the reads of such a sample have no file-order numbers)
    std::vector<std::string> mapped_paths;
    bool fastx_unordered = false;
    bool needs_reset = false; // reduce_devices failed half way: the devices' vectors are in no defined state
    Selection subsample, dedup; // drprg_hip_subsample, drprg_hip_dedup
    // mate overlap: drprg_hip_begin_mates was called (the files mapped since are side 2); the last drprg_hip_pair_overlap's twelve counts
    // and its chosen shift per source pair
    bool mates_begun = false, pair_done = false;
    uint64_t pair_counts[12] = {};
    std::vector<int32_t> pair_shifts;
    // mate merging: that call merged (drprg_hip_set_pair_merge was on), and its eight counts
    bool pair_merge_done = false;
    uint64_t pair_merge_counts[8] = {};
    // duplicate pairs: the last drprg_hip_dedup_pairs (its flags; counts is not used), and its forty words: eight counts, 32 levels
    Selection pair_dedup;
    uint64_t pair_dedup_words[40] = {};
    // What the read filter has counted: added to by the submitters of drprg_hip_map_fastx, one per device, under filter_mu.  The blocks'
    // outcomes summed: drprg_hip_read_filter_info, and in .trim / .adapter / .front drprg_hip_read_trim_info,
    // drprg_hip_adapter_trim_info and drprg_hip_front_adapter_info, in .mask drprg_hip_base_mask_info, in .decoy drprg_hip_decoy_info, in
    // .poly drprg_hip_poly_trim_info, in .cplx drprg_hip_complexity_info.
    Mapper::FilterOutcome filter_counts;
    // read statistics (drprg_hip_set_read_stats): a pass of drprg_hip_map_fastx ran under a prep setting or a depth cap, so the prepared
    // snapshot was counted on its own; false: it is the raw snapshot by definition (drprg_hip_read_stats_info says which)
    bool stats_prepared = false;
    MapCounters extra_counts; // what devices 1 .. ndev-1 counted (reduce_devices folds them in when it folds their coverage)
};
} // namespace drprg

struct drprg_hip_ctx {
    drprg::PrgIndex index;
    std::unique_ptr<drprg::Mapper> mapper; // null for a host-only context; device 0 of a multi-device context
    std::vector<std::unique_ptr<drprg::Mapper>> extra; // devices 1 .. ndev-1 of drprg_hip_open_multi (map_fastx shards the reads over all)
    drprg::MapParams params;
    std::string prg_file;
    std::string last_error;
    drprg::SampleState sample;
    // ---- settings: a reset keeps them ----
    uint64_t max_covg = ~0ull; // drprg_hip_set_max_covg (off)
    int threads = 4; // parser threads of drprg_hip_map_fastx
    bool packed_input = false; // drprg_hip_set_input_format: map_fastx packs the reads to 2 bits on the parser threads
    bool ordered_ingest = false; // drprg_hip_set_ordered_ingest
    // drprg_hip_set_read_filter; the settings of drprg_hip_set_read_trim, drprg_hip_set_adapters*, drprg_hip_set_base_mask,
    // drprg_hip_set_poly_trim and drprg_hip_set_min_complexity ride in it too
    drprg::Mapper::ReadFilter read_filter;
    std::mutex filter_mu; // guards sample.filter_counts
    drprg::Mapper::PairSetting pair; // drprg_hip_set_pair_overlap
    bool dedup_pairs = false;        // drprg_hip_set_dedup_pairs
    // ---- results of the last calls: a reset keeps them ----
    uint32_t ginfo[4] = { 0, 0, 0, 0 };
    std::vector<drprg::VcfRecord> last_records; // of the last drprg_hip_genotype (drprg_hip_genotype_alleles)
    drprg::CoverageModel last_model;            // of the last drprg_hip_genotype (drprg_hip_coverage_model)
    size_t last_dropped = 0;                    // loci it dropped for a bare best path
    // the last drprg_hip_discover_reads: what drprg_hip_update_prg applies, and whether it took its reads from HBM
    drprg::GenotypeResult last_discover;
    std::vector<drprg::NovelVariant> last_variants;
    bool last_discover_resident = false;
    // multi-device context: RCCL communicators of its devices (created on first use; empty when RCCL is not used)
    std::vector<drprg::Rccl::Comm> comms;
    std::string reduce_how; // how the last drprg_hip_reduce / drprg_hip_allreduce summed the vectors (drprg_hip_reduce_info)
    drprg_hip_ctx() { drprg::pin_pool_context_opened(); }
    ~drprg_hip_ctx()
    {
        if (!comms.empty())
            if (const drprg::Rccl* r = drprg::Rccl::get())
                for (drprg::Rccl::Comm c : comms)
                    if (c) (void)r->CommDestroy(c);
        drprg::pin_pool_context_closed();
    }
};

#define API_BEGIN(ctx) if (!(ctx)) return DRPRG_EINVAL; try {
#define API_FAIL(ctx, what, code) { (ctx)->last_error = (what); return (code); }
#define API_END(ctx)                                                                 \
    }                                                                                \
    catch (const drprg::Error& e) API_FAIL(ctx, e.what(), e.code)                    \
    catch (const std::bad_alloc&) API_FAIL(ctx, "out of host memory", DRPRG_ENOMEM)  \
    catch (const std::exception& e) API_FAIL(ctx, e.what(), DRPRG_EIO)               \
    return DRPRG_OK;

namespace drprg {
int thread_error(int code, const std::string& what); // capi.cpp: `what` becomes this thread's drprg_hip_last_error(NULL); returns code

inline Mapper& need_mapper(drprg_hip_ctx* ctx)
{
    if (!ctx->mapper) throw Error(DRPRG_ENODEV, "host-only context: the hot path runs on a HIP device only (no CPU fallback)");
    return *ctx->mapper;
}

inline std::vector<Mapper*> mappers_of(drprg_hip_ctx* ctx)
{
    std::vector<Mapper*> all;
    if (ctx->mapper) all.push_back(ctx->mapper.get());
    for (auto& e : ctx->extra) all.push_back(e.get());
    return all;
}

void sync_host_coverage(drprg_hip_ctx* ctx);               // capi.cpp: the host copy made valid (downloaded if need be)
void reduce_devices(drprg_hip_ctx* ctx);                   // capi_reduce.cpp: the devices' vectors summed into the first device
bool reads_resident(drprg_hip_ctx* ctx, const char* path); // capi_prep.cpp: do the reads in HBM stand for the file (null: for whatever was mapped)?
} // namespace drprg

#pragma GCC visibility pop
