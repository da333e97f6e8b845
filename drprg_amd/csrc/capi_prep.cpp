// capi_prep.cpp -- read preparation (filter, trimming, adapters, poly tails, read complexity, base mask, decoy screen: settings, counts, device
// entries) and the resident sample
// (keep, map from another context, select, subsample, dedup).
#include "capi_ctx.h"
#include "fastx.h"
#include "read_stats_host.h"
#include <cstdio>
#include "read_qual_piece.h"
#include "read_trim_piece.h"
#include <algorithm>
#include <atomic>
#include <cstring>

using namespace drprg;

extern "C" {

int drprg_hip_set_read_filter(drprg_hip_ctx* ctx, uint64_t min_len, uint64_t max_len, uint32_t min_qual_milli)
{
    API_BEGIN(ctx)
    if (max_len != 0 && max_len < min_len) throw Error(DRPRG_EINVAL, "read filter: the longest read allowed is shorter than the shortest");
    if (min_qual_milli > dev::RQ_MAX_QUAL_MILLI) throw Error(DRPRG_EINVAL, "read filter: a mean quality above 93 cannot be asked for");
    Mapper::ReadFilter f = ctx->read_filter; // (the trim settings ride along: drprg_hip_set_read_trim)
    f.min_len = min_len; f.max_len = max_len; f.min_qual_milli = min_qual_milli;
    f.T = min_qual_milli ? dev::rq_threshold(min_qual_milli) : 0;
    ctx->read_filter = f;
    API_END(ctx)
}

int drprg_hip_read_filter_info(drprg_hip_ctx* ctx, uint64_t out[8])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    std::lock_guard<std::mutex> g(ctx->filter_mu);
    const Mapper::FilterOutcome& t = ctx->sample.filter_counts;
    out[0] = t.reads_seen; out[1] = t.bases_seen; out[2] = t.dropped_short; out[3] = t.dropped_long; out[4] = t.dropped_lowq;
    out[5] = t.reads_kept; out[6] = t.bases_kept; out[7] = ctx->read_filter.T;
    API_END(ctx)
}

int drprg_hip_read_filter_device(drprg_hip_ctx* ctx, const void* d_qual, uint32_t qual_bias, const void* d_offsets, uint64_t n_reads, uint64_t n_bases,
    void* d_sums, void* d_flags, uint64_t out[4], void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    if (qual_bias != 0 && qual_bias != 33) throw Error(DRPRG_EINVAL, "read filter: the quality bias is 33 (FASTQ) or 0 (BAM)");
    uint64_t res[8];
    m.read_filter_device(ctx->read_filter, (const uint8_t*)d_qual, qual_bias, (const uint64_t*)d_offsets, n_reads, n_bases, (unsigned long long*)d_sums,
        (uint8_t*)d_flags, res, (hipStream_t)hip_stream);
    out[0] = res[dev::RF_KEPT_READS]; out[1] = res[dev::RF_KEPT_BASES]; out[2] = res[dev::RF_BAD_AT]; out[3] = 0;
    if (res[dev::RF_OFFSETS]) throw Error(DRPRG_EINVAL, "read filter: the offsets do not ascend to n_bases");
    if (res[dev::RF_BAD_AT]) throw Error(DRPRG_EFORMAT, "a base quality outside 0..93 at quality byte " + std::to_string(res[dev::RF_BAD_AT] - 1));
    API_END(ctx)
}

// ---- read trimming (the rule: include/drprg_hip.h "read trimming") ---------------------------------------------------------------
int drprg_hip_set_read_trim(drprg_hip_ctx* ctx, uint64_t front, uint64_t tail, uint32_t qual_milli, uint32_t window)
{
    API_BEGIN(ctx)
    if (qual_milli > dev::RT_MAX_QUAL_MILLI) throw Error(DRPRG_EINVAL, "read trimming: a quality above 93 cannot be asked for");
    if (window > dev::RT_MAX_WINDOW) throw Error(DRPRG_EINVAL, "read trimming: the window is 1..32 bases");
    if (window != 0 && qual_milli == 0) throw Error(DRPRG_EINVAL, "read trimming: a window without a quality (--trim-window without --trim-qual)");
    ctx->read_filter.trim_front = front; ctx->read_filter.trim_tail = tail; ctx->read_filter.trim_qual_milli = qual_milli;
    ctx->read_filter.trim_window = qual_milli ? (window ? window : dev::RT_DEFAULT_WINDOW) : 0;
    API_END(ctx)
}

int drprg_hip_read_trim_info(drprg_hip_ctx* ctx, uint64_t out[8])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    std::lock_guard<std::mutex> g(ctx->filter_mu);
    const Mapper::TrimOutcome& t = ctx->sample.filter_counts.trim;
    out[0] = t.reads_seen; out[1] = t.bases_seen; out[2] = t.reads_lost_base; out[3] = t.cut_front; out[4] = t.cut_tail;
    out[5] = t.qcut_front; out[6] = t.qcut_tail; out[7] = t.emptied;
    API_END(ctx)
}

int drprg_hip_read_trim_device(drprg_hip_ctx* ctx, const void* d_qual, uint32_t qual_bias, const void* d_offsets, const void* d_rev, uint64_t n_reads,
    uint64_t n_bases, void* d_begin, void* d_end, uint64_t out[4], void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    if (qual_bias != 0 && qual_bias != 33) throw Error(DRPRG_EINVAL, "read trimming: the quality bias is 33 (FASTQ) or 0 (BAM)");
    uint64_t res[9];
    m.read_trim_device(ctx->read_filter, (const uint8_t*)d_qual, qual_bias, (const uint64_t*)d_offsets, (const uint8_t*)d_rev, n_reads, n_bases,
        (uint64_t*)d_begin, (uint64_t*)d_end, res, (hipStream_t)hip_stream);
    const bool bad_offsets = res[dev::RT_BAD_AT] == ~0ull;
    out[0] = res[dev::RT_KEPT_BASES]; out[1] = res[dev::RT_LOST_READS]; out[2] = bad_offsets ? 0 : res[dev::RT_BAD_AT]; out[3] = 0;
    if (bad_offsets) throw Error(DRPRG_EINVAL, "read trimming: the offsets do not ascend to n_bases (or a read is longer than 2^31 bases)");
    if (res[dev::RT_BAD_AT]) throw Error(DRPRG_EFORMAT, "a base quality outside 0..93 at quality byte " + std::to_string(res[dev::RT_BAD_AT] - 1));
    API_END(ctx)
}

// ---- adapter trimming (the rule: include/drprg_hip.h "adapter trimming") ----------------------------------------------------------
// one side's list into the kernels' form; shortest: lowered to the shortest adapter's length
static dev::AdapterSet adapter_list(const char* const* seqs, uint32_t n, uint32_t& shortest)
{
    dev::AdapterSet ad {};
    if (n == 0) return ad;
    if (!seqs) throw Error(DRPRG_EINVAL, "adapter trimming: null adapter list");
    if (n > dev::AD_MAX_ADAPTERS) throw Error(DRPRG_EINVAL, "adapter trimming: at most 4 adapters");
    for (uint32_t a = 0; a < n; ++a) {
        if (!seqs[a]) throw Error(DRPRG_EINVAL, "adapter trimming: null adapter");
        const size_t m = std::strlen(seqs[a]);
        if (m < 1 || m > dev::AD_MAX_LEN) throw Error(DRPRG_EINVAL, "adapter trimming: an adapter is 1..64 letters long");
        for (size_t j = 0; j < m; ++j) {
            const uint32_t l = dev::ad_letter((uint8_t)seqs[a][j]);
            if (l > 3) throw Error(DRPRG_EINVAL, "adapter trimming: an adapter holds the letters ACGT (either case) and no other");
            (j < 32 ? ad.lo[a] : ad.hi[a]) |= (uint64_t)l << (2 * (j & 31));
        }
        ad.len[a] = (uint32_t)m;
        if (m > ad.max_len) ad.max_len = (uint32_t)m;
        if (m < shortest) shortest = (uint32_t)m;
    }
    ad.n = n;
    return ad;
}

static void clear_adapters(drprg_hip_ctx* ctx)
{
    Mapper::ReadFilter& f = ctx->read_filter;
    f.adapters = dev::AdapterSet {};
    f.front_adapters = dev::AdapterSet {};
    f.eq3 = f.eq5 = dev::AdapterEq {};
    f.adapter_indels = false;
}

// Behind both settings entries (the plain rule is the second form without a 5' list and without flags).  overlap_refusal: what a
// minimum overlap above the shortest adapter is refused with, in the entry's own words.
static int set_adapters(drprg_hip_ctx* ctx, const char* const* seqs3, uint32_t n3, const char* const* seqs5, uint32_t n5, uint32_t error_milli,
    uint32_t min_overlap, uint32_t flags, const char* overlap_refusal)
{
    API_BEGIN(ctx)
    if (flags & ~dev::AE_FLAG_INDELS) throw Error(DRPRG_EINVAL, "adapter trimming: unknown flag bits");
    if (n3 == 0 && n5 == 0) { // cleared
        clear_adapters(ctx);
        return DRPRG_OK;
    }
    const bool indels = (flags & dev::AE_FLAG_INDELS) != 0;
    if (n5 && !indels) throw Error(DRPRG_EINVAL, "adapter trimming: 5' adapters exist only under the indel rule (flag bit 0)");
    if (error_milli > dev::AD_MAX_ERROR_MILLI) throw Error(DRPRG_EINVAL, "adapter trimming: the error rate is 0..0.5");
    uint32_t shortest = dev::AD_MAX_LEN;
    dev::AdapterSet ad3 = adapter_list(seqs3, n3, shortest), ad5 = adapter_list(seqs5, n5, shortest);
    if (min_overlap > shortest) throw Error(DRPRG_EINVAL, overlap_refusal);
    const uint32_t O = min_overlap ? min_overlap : std::min(dev::AD_DEFAULT_MIN_OVERLAP, shortest);
    if (ad3.n) { ad3.error_milli = error_milli; ad3.min_overlap = O; }
    if (ad5.n) { ad5.error_milli = error_milli; ad5.min_overlap = O; }
    clear_adapters(ctx);
    Mapper::ReadFilter& f = ctx->read_filter;
    f.adapters = ad3;
    if (indels) {
        f.adapter_indels = true;
        f.front_adapters = dev::ae_reversed(ad5);
        f.eq3 = dev::ae_make_eq(f.adapters);
        f.eq5 = dev::ae_make_eq(f.front_adapters);
    }
    API_END(ctx)
}

int drprg_hip_set_adapters(drprg_hip_ctx* ctx, const char* const* seqs, uint32_t n, uint32_t error_milli, uint32_t min_overlap)
{
    return set_adapters(ctx, seqs, n, nullptr, 0, error_milli, min_overlap, 0, "adapter trimming: the minimum overlap is 1..the length of the shortest adapter");
}

int drprg_hip_set_adapters2(drprg_hip_ctx* ctx, const char* const* seqs3, uint32_t n3, const char* const* seqs5, uint32_t n5, uint32_t error_milli,
    uint32_t min_overlap, uint32_t flags)
{
    return set_adapters(ctx, seqs3, n3, seqs5, n5, error_milli, min_overlap, flags,
        "adapter trimming: the minimum overlap is 1..the length of the shortest adapter of either side");
}

// behind drprg_hip_adapter_trim_info (the 3' side's counts) and drprg_hip_front_adapter_info (the 5' side's)
static int adapter_info(drprg_hip_ctx* ctx, bool front, uint64_t out[5])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    std::lock_guard<std::mutex> g(ctx->filter_mu);
    const Mapper::AdapterOutcome& t = front ? ctx->sample.filter_counts.front : ctx->sample.filter_counts.adapter;
    out[0] = t.reads_seen; out[1] = t.bases_seen; out[2] = t.reads_cut; out[3] = t.bases_cut; out[4] = t.reads_emptied;
    API_END(ctx)
}

int drprg_hip_adapter_trim_info(drprg_hip_ctx* ctx, uint64_t out[5]) { return adapter_info(ctx, false, out); }
int drprg_hip_front_adapter_info(drprg_hip_ctx* ctx, uint64_t out[5]) { return adapter_info(ctx, true, out); }

// Behind both adapter device entries.  n_out: the words of the result handed out (5: the 3' side's counts; 10: both sides').  plain_only: the
// first form knows the mismatch rule's 3' adapters alone -- d_begin is left as it is, the 5' side's counts stay zero -- and refuses the rest.
static int adapter_trim_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, const void* d_begin, void* d_end, uint64_t* out, int n_out, bool plain_only, void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    if (d_text && d_words) throw Error(DRPRG_EINVAL, "adapter trimming: the bases come as text or as packed words, not both");
    if (plain_only && n_reads && !ctx->read_filter.adapters.n) throw Error(DRPRG_EINVAL, "adapter trimming: no adapter is set (drprg_hip_set_adapters)");
    if (plain_only && n_reads && ctx->read_filter.adapter_indels)
        throw Error(DRPRG_EINVAL, "adapter trimming: the indel rule is set (drprg_hip_set_adapters2); it runs through drprg_hip_adapter_trim_device2");
    uint64_t res[11];
    m.adapter_trim_device(ctx->read_filter, (const uint8_t*)d_text, (const uint32_t*)d_words, (const uint64_t*)d_npos, n_npos, (const uint64_t*)d_offsets, n_reads,
        n_bases, (uint64_t*)d_begin, (uint64_t*)d_end, res, (hipStream_t)hip_stream);
    for (int i = 0; i < n_out; ++i) out[i] = res[i];
    if (res[10]) throw Error(DRPRG_EINVAL, "adapter trimming: the offsets do not ascend to n_bases, or a range does not lie inside its read");
    API_END(ctx)
}

int drprg_hip_adapter_trim_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, const void* d_begin, void* d_end, uint64_t out[5], void* hip_stream)
{
    return adapter_trim_device(ctx, d_text, d_words, d_npos, n_npos, d_offsets, n_reads, n_bases, d_begin, d_end, out, 5, true, hip_stream);
}

int drprg_hip_adapter_trim_device2(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, void* d_begin, void* d_end, uint64_t out[10], void* hip_stream)
{
    return adapter_trim_device(ctx, d_text, d_words, d_npos, n_npos, d_offsets, n_reads, n_bases, d_begin, d_end, out, 10, false, hip_stream);
}

// ---- poly tails (the rule: include/drprg_hip.h "poly tails") ------------------------------------------------------------------------
int drprg_hip_set_poly_trim(drprg_hip_ctx* ctx, const char* letters, uint32_t min_len)
{
    API_BEGIN(ctx)
    if (!letters || !*letters) { // cleared
        ctx->read_filter.poly_letters = ctx->read_filter.poly_min_len = 0;
        return DRPRG_OK;
    }
    static const char acgt[] = "ACGT";
    uint32_t set = 0;
    for (const char* c = letters; *c; ++c) {
        const char* at = (*c & 0x40) ? std::strchr(acgt, *c & 0xDF) : nullptr;
        if (!at) throw Error(DRPRG_EINVAL, "poly-tail trimming: the letters are ACGT (either case) and no other");
        const uint32_t bit = 1u << (at - acgt);
        if (set & bit) throw Error(DRPRG_EINVAL, "poly-tail trimming: a letter is named once");
        set |= bit;
    }
    if (min_len < dev::PT_MIN_LEN_LO || min_len > dev::PT_MIN_LEN_HI) throw Error(DRPRG_EINVAL, "poly-tail trimming: the shortest tail cut is 2..255 bases long");
    ctx->read_filter.poly_letters = set; // (they ride in the settings every device's blocks are prepared under, like the trim settings)
    ctx->read_filter.poly_min_len = min_len;
    API_END(ctx)
}

int drprg_hip_poly_trim_info(drprg_hip_ctx* ctx, uint64_t out[5])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    std::lock_guard<std::mutex> g(ctx->filter_mu);
    const Mapper::PolyOutcome& t = ctx->sample.filter_counts.poly;
    out[0] = t.reads_seen; out[1] = t.bases_seen; out[2] = t.reads_cut; out[3] = t.bases_cut; out[4] = t.reads_emptied;
    API_END(ctx)
}

int drprg_hip_poly_trim_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, const void* d_begin, void* d_end, uint64_t out[5], void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    if (d_text && d_words) throw Error(DRPRG_EINVAL, "poly-tail trimming: the bases come as text or as packed words, not both");
    uint64_t res[6];
    m.poly_trim_device(ctx->read_filter, (const uint8_t*)d_text, (const uint32_t*)d_words, (const uint64_t*)d_npos, n_npos, (const uint64_t*)d_offsets, n_reads,
        n_bases, (const uint64_t*)d_begin, (uint64_t*)d_end, res, (hipStream_t)hip_stream);
    for (int i = 0; i < 5; ++i) out[i] = res[i];
    if (res[5]) throw Error(DRPRG_EINVAL, "poly-tail trimming: the offsets do not ascend to n_bases, or a range does not lie inside its read");
    API_END(ctx)
}

// ---- the low-complexity filter (the rule: include/drprg_hip.h "read complexity") ----------------------------------------------------
int drprg_hip_set_min_complexity(drprg_hip_ctx* ctx, uint32_t percent)
{
    API_BEGIN(ctx)
    if (percent > 100) throw Error(DRPRG_EINVAL, "read complexity: the threshold is a percentage, 1..100 (0 clears it)");
    ctx->read_filter.min_complexity = percent;
    API_END(ctx)
}

int drprg_hip_complexity_info(drprg_hip_ctx* ctx, uint64_t out[4])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    std::lock_guard<std::mutex> g(ctx->filter_mu);
    const Mapper::ComplexityOutcome& t = ctx->sample.filter_counts.cplx;
    out[0] = t.reads_judged; out[1] = t.bases_judged; out[2] = t.reads_dropped; out[3] = t.bases_dropped;
    API_END(ctx)
}

int drprg_hip_complexity_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, void* d_diff, void* d_flags, uint64_t out[2], void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    if (d_text && d_words) throw Error(DRPRG_EINVAL, "read complexity: the bases come as text or as packed words, not both");
    uint64_t res[3];
    m.complexity_device(ctx->read_filter, (const uint8_t*)d_text, (const uint32_t*)d_words, (const uint64_t*)d_npos, n_npos, (const uint64_t*)d_offsets, n_reads,
        n_bases, (uint32_t*)d_diff, (uint8_t*)d_flags, res, (hipStream_t)hip_stream);
    out[0] = res[0]; out[1] = res[1];
    if (res[2]) throw Error(DRPRG_EINVAL, "read complexity: the offsets do not ascend from 0 to n_bases");
    API_END(ctx)
}

// ---- base masking (the rule: include/drprg_hip.h "base masking") -------------------------------------------------------------------
int drprg_hip_set_base_mask(drprg_hip_ctx* ctx, uint32_t min_qual)
{
    API_BEGIN(ctx)
    if (min_qual > 93) throw Error(DRPRG_EINVAL, "base masking: a quality above 93 cannot be asked for");
    ctx->read_filter.mask_qual = min_qual; // (it rides in the settings every device's blocks are prepared under, like the trim settings)
    API_END(ctx)
}

int drprg_hip_base_mask_info(drprg_hip_ctx* ctx, uint64_t out[5])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    std::lock_guard<std::mutex> g(ctx->filter_mu);
    const Mapper::MaskOutcome& t = ctx->sample.filter_counts.mask;
    out[0] = t.reads_seen; out[1] = t.bases_seen; out[2] = t.reads_masked; out[3] = t.bases_masked; out[4] = t.bases_already_unknown;
    API_END(ctx)
}

int drprg_hip_base_mask_device(drprg_hip_ctx* ctx, const void* d_qual, uint32_t qual_bias, const void* d_offsets, const void* d_rev, uint64_t n_reads,
    uint64_t n_bases, void* d_text, void* d_words, const void* d_npos, uint64_t n_npos, void* d_npos_out, uint64_t npos_cap, uint64_t out[6], void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    if (qual_bias != 0 && qual_bias != 33) throw Error(DRPRG_EINVAL, "base masking: the quality bias is 33 (FASTQ) or 0 (BAM)");
    if (d_text && d_words) throw Error(DRPRG_EINVAL, "base masking: the bases come as text or as packed words, not both");
    uint64_t res[8];
    m.base_mask_device(ctx->read_filter, (const uint8_t*)d_qual, qual_bias, (const uint64_t*)d_offsets, (const uint8_t*)d_rev, n_reads, n_bases, (uint8_t*)d_text,
        (uint32_t*)d_words, (const uint64_t*)d_npos, n_npos, (uint64_t*)d_npos_out, npos_cap, res, (hipStream_t)hip_stream);
    for (int i = 0; i < 6; ++i) out[i] = res[i];
    if (res[7]) throw Error(DRPRG_EINVAL, "base masking: the offsets do not run from 0 to n_bases");
    if (res[6]) throw Error(DRPRG_EFORMAT, "a base quality outside 0..93 at quality byte " + std::to_string(res[6] - 1));
    if (res[5] > npos_cap || (res[5] && !d_npos_out))
        throw Error(DRPRG_EOVERFLOW, "base masking: the list behind the mask holds " + std::to_string(res[5]) + " positions, the buffer " + std::to_string(d_npos_out ? npos_cap : 0));
    API_END(ctx)
}

// ---- read statistics (the rule: include/drprg_hip.h "read statistics"; the layout: read_stats_words.h) ------------------------------------
uint64_t drprg_hip_read_stats_words(void) { return dev::RS_WORDS; }

int drprg_hip_read_stats_layout(uint64_t out[13])
{
    if (!out) return DRPRG_EINVAL;
    const uint64_t v[13] = { dev::RS_WORDS, dev::RS_LEN_READS, dev::RS_LEN_BASES, dev::RS_CYC_BASE, dev::RS_CYC_QSUM, dev::RS_QUAL_HIST, dev::RS_READQ_HIST,
        dev::RS_GC_HIST, dev::RS_LEN_BINS, dev::RS_CYCLES, dev::RS_COLS, dev::RS_QUALS, dev::RS_GC_BINS };
    for (int i = 0; i < 13; ++i) out[i] = v[i];
    return DRPRG_OK;
}

int drprg_hip_set_read_stats(drprg_hip_ctx* ctx, int mode)
{
    API_BEGIN(ctx)
    if (mode < 0 || mode > 2) throw Error(DRPRG_EINVAL, "read statistics: the mode is 0 (off), 1 (with qualities) or 2 (without)");
    ctx->read_filter.read_stats = (uint32_t)mode; // (it rides in the settings every device's blocks are prepared under, like the trim settings)
    API_END(ctx)
}

// one snapshot of the context: its devices' folded (which 1 on a sample no prep setting or cap touched: the raw one)
static void read_stats_snapshot(drprg_hip_ctx* ctx, int which, std::vector<uint64_t>& w)
{
    if (which == 1 && !ctx->sample.stats_prepared) which = 0;
    w.assign(dev::RS_WORDS, 0);
    w[dev::RS_MIN_LEN] = ~0ull;
    std::vector<uint64_t> one(dev::RS_WORDS);
    for (Mapper* m : mappers_of(ctx)) {
        m->read_stats(which, one.data());
        rs_fold(w.data(), one.data());
    }
    rs_finish(w.data());
}

int drprg_hip_read_stats_info(drprg_hip_ctx* ctx, int which, uint64_t* out, uint64_t n_words)
{
    API_BEGIN(ctx)
    need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    if (which != 0 && which != 1) throw Error(DRPRG_EINVAL, "read statistics: the snapshot is 0 (raw) or 1 (prepared)");
    if (n_words < dev::RS_WORDS) throw Error(DRPRG_EINVAL, "read statistics: a snapshot holds " + std::to_string(dev::RS_WORDS) + " words (drprg_hip_read_stats_words), the buffer " + std::to_string(n_words));
    std::vector<uint64_t> w;
    read_stats_snapshot(ctx, which, w);
    std::memcpy(out, w.data(), dev::RS_WORDS * sizeof(uint64_t));
    API_END(ctx)
}

int drprg_hip_read_stats_prepared_is_raw(drprg_hip_ctx* ctx)
{
    if (!ctx) return DRPRG_EINVAL;
    return ctx->sample.stats_prepared ? 0 : 1;
}

int drprg_hip_read_stats_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_qual, uint32_t qual_bias,
    const void* d_offsets, const void* d_rev, uint64_t n_reads, uint64_t n_bases, const void* d_flags, uint64_t take, uint64_t* out, uint64_t n_words, void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    if (n_words < dev::RS_WORDS) throw Error(DRPRG_EINVAL, "read statistics: a snapshot holds " + std::to_string(dev::RS_WORDS) + " words (drprg_hip_read_stats_words), the buffer " + std::to_string(n_words));
    if (qual_bias != 0 && qual_bias != 33) throw Error(DRPRG_EINVAL, "read statistics: the quality bias is 33 (FASTQ) or 0 (BAM)");
    if (d_text && d_words) throw Error(DRPRG_EINVAL, "read statistics: the bases come as text or as packed words, not both");
    uint64_t res[2];
    m.read_stats_device((const uint8_t*)d_text, (const uint32_t*)d_words, (const uint64_t*)d_npos, n_npos, (const uint8_t*)d_qual, qual_bias, (const uint64_t*)d_offsets,
        (const uint8_t*)d_rev, n_reads, n_bases, (const uint8_t*)d_flags, take, out, res, (hipStream_t)hip_stream);
    if (res[1]) throw Error(DRPRG_EINVAL, "read statistics: the offsets do not ascend from 0 to n_bases");
    if (res[0]) throw Error(DRPRG_EFORMAT, "a base quality outside 0..93 at quality byte " + std::to_string(res[0] - 1));
    API_END(ctx)
}

int drprg_hip_write_qc_json(drprg_hip_ctx* ctx, const char* path, const char* sample)
{
    API_BEGIN(ctx)
    need_mapper(ctx);
    if (!path) throw Error(DRPRG_EINVAL, "null path");
    const Mapper::ReadFilter& f = ctx->read_filter;
    if (!f.read_stats) throw Error(DRPRG_EINVAL, "read statistics are not set (drprg_hip_set_read_stats)");
    std::vector<uint64_t> raw, prepared;
    read_stats_snapshot(ctx, 0, raw);
    read_stats_snapshot(ctx, 1, prepared);
    QcReport r;
    r.sample = sample ? sample : "";
    r.with_qual = f.read_stats == 1;
    r.prepared_is_raw = !ctx->sample.stats_prepared;
    r.raw = raw.data();
    r.prepared = prepared.data();
    r.settings = { { "max_covg", ctx->max_covg >= 0xFFFFFFFFull ? 0xFFFFFFFFull : ctx->max_covg } /* 4294967295: off */, { "min_read_len", f.min_len },
        { "max_read_len", f.max_len }, { "min_read_qual_milli", f.min_qual_milli }, { "trim_front", f.trim_front }, { "trim_tail", f.trim_tail },
        { "trim_qual_milli", f.trim_qual_milli }, { "trim_window", f.trim_window }, { "adapters", f.adapters.n }, { "front_adapters", f.front_adapters.n },
        { "adapter_indels", f.adapter_indels ? 1u : 0u }, { "poly_letters", f.poly_letters }, { "poly_min_len", f.poly_min_len }, { "mask_qual", f.mask_qual },
        { "min_complexity", f.min_complexity }, { "decoy_k", f.decoy_k }, { "decoy_frac_milli", f.decoy_frac_milli }, { "decoy_min_kmers", f.decoy_min_kmers },
        { "packed_input", ctx->packed_input ? 1u : 0u } };
    // the counters every stage keeps, as its *_info entry returns them
    const auto stage = [&](const char* name, int (*info)(drprg_hip_ctx*, uint64_t*), size_t n) {
        std::vector<uint64_t> v(n, 0);
        if (int rc = info(ctx, v.data())) throw Error(rc, ctx->last_error);
        r.stages.emplace_back(name, std::move(v));
    };
    stage("read_trim", drprg_hip_read_trim_info, 8);
    stage("adapter_trim", drprg_hip_adapter_trim_info, 5);
    stage("front_adapter", drprg_hip_front_adapter_info, 5);
    stage("poly_trim", drprg_hip_poly_trim_info, 5);
    stage("base_mask", drprg_hip_base_mask_info, 5);
    stage("read_filter", drprg_hip_read_filter_info, 8);
    stage("complexity", drprg_hip_complexity_info, 4);
    stage("decoy", drprg_hip_decoy_info, 8);
    stage("max_covg", drprg_hip_max_covg_info, 4);
    const Selection& dd = ctx->sample.dedup;
    const Selection& ss = ctx->sample.subsample;
    if (ctx->sample.pair_done) // (only when the stage ran: a report without --mate stays byte for byte what it was)
        r.stages.emplace_back("pair_overlap", std::vector<uint64_t>(ctx->sample.pair_counts, ctx->sample.pair_counts + 12));
    if (ctx->sample.pair_merge_done) // (likewise: only when the stage ran with the switch on)
        r.stages.emplace_back("pair_merge", std::vector<uint64_t>(ctx->sample.pair_merge_counts, ctx->sample.pair_merge_counts + 8));
    if (ctx->sample.pair_dedup.done) // (likewise: the eight counts, then the 32 duplication levels)
        r.stages.emplace_back("pair_dedup", std::vector<uint64_t>(ctx->sample.pair_dedup_words, ctx->sample.pair_dedup_words + 40));
    r.stages.emplace_back("dedup", dd.done ? std::vector<uint64_t>(dd.counts, dd.counts + 4) : std::vector<uint64_t>());
    r.stages.emplace_back("subsample", ss.done ? std::vector<uint64_t>(ss.counts, ss.counts + 4) : std::vector<uint64_t>());
    const std::string text = qc_json(r);
    FILE* fp = std::fopen(path, "wb");
    if (!fp) throw Error(DRPRG_EIO, std::string("cannot write ") + path);
    const bool ok = std::fwrite(text.data(), 1, text.size(), fp) == text.size();
    if (std::fclose(fp) != 0 || !ok) throw Error(DRPRG_EIO, std::string("cannot write ") + path);
    API_END(ctx)
}

// ---- the decoy screen (the rule: include/drprg_hip.h "decoy screen") ----------------------------------------------------------------
static void clear_decoy(drprg_hip_ctx* ctx)
{
    Mapper::ReadFilter& f = ctx->read_filter;
    f.decoy_k = f.decoy_frac_milli = f.decoy_min_kmers = 0;
    f.decoy_id = 0;
    for (Mapper* m : mappers_of(ctx)) m->clear_decoy();
}

// every record of the files, one 'N' between two records (no window spans it); windows: those of the records, whatever letters they hold
static std::vector<uint8_t> decoy_text(const char* const* paths, uint32_t n, uint32_t k, uint64_t& windows)
{
    std::vector<uint8_t> text;
    windows = 0;
    for (uint32_t i = 0; i < n; ++i) {
        FastxReader rd(paths[i]);
        ReadBatch batch;
        while (rd.next_batch(batch, 1u << 20, 1ull << 28)) {
            for (uint64_t r = 0; r < batch.n_reads(); ++r) {
                const uint64_t len = batch.offsets[r + 1] - batch.offsets[r];
                if (len < k) continue; // (adds nothing)
                windows += len - k + 1;
                if (windows > dev::DC_MAX_WINDOWS) throw Error(DRPRG_EOVERFLOW, "decoy screen: the decoy files hold more than 2^31 - 1 windows");
                if (!text.empty()) text.push_back('N');
                text.insert(text.end(), batch.bases.begin() + (long)batch.offsets[r], batch.bases.begin() + (long)batch.offsets[r + 1]);
            }
        }
    }
    return text;
}

int drprg_hip_set_decoy(drprg_hip_ctx* ctx, const char* const* fasta_paths, uint32_t n, uint32_t k, uint32_t min_frac_milli, uint32_t min_kmers)
{
    API_BEGIN(ctx)
    static std::atomic<uint64_t> sets { 0 };
    clear_decoy(ctx); // (whatever happens below, the set that was is gone)
    if (n == 0) return DRPRG_OK;
    need_mapper(ctx);
    if (n > dev::DC_MAX_FILES) throw Error(DRPRG_EINVAL, "decoy screen: at most 8 decoy files");
    if (!fasta_paths) throw Error(DRPRG_EINVAL, "decoy screen: null list of decoy files");
    for (uint32_t i = 0; i < n; ++i)
        if (!fasta_paths[i]) throw Error(DRPRG_EINVAL, "decoy screen: null decoy file name");
    if (k == 0) k = dev::DC_DEFAULT_K;
    if (k < dev::DC_MIN_K || k > dev::DC_MAX_K) throw Error(DRPRG_EINVAL, "decoy screen: the k-mer length is 9..31");
    if (min_frac_milli > 1000) throw Error(DRPRG_EINVAL, "decoy screen: the fraction is at most 1");
    uint64_t windows = 0;
    const std::vector<uint8_t> text = decoy_text(fasta_paths, n, k, windows);
    const uint64_t set = ++sets;
    try {
        for (Mapper* m : mappers_of(ctx)) m->set_decoy(text, windows, k, set);
    } catch (...) {
        clear_decoy(ctx);
        throw;
    }
    Mapper::ReadFilter& f = ctx->read_filter;
    f.decoy_k = k;
    f.decoy_frac_milli = min_frac_milli ? min_frac_milli : dev::DC_DEFAULT_FRAC_MILLI;
    f.decoy_min_kmers = min_kmers ? min_kmers : dev::DC_DEFAULT_MIN_KMERS;
    f.decoy_id = set;
    API_END(ctx)
}

int drprg_hip_decoy_info(drprg_hip_ctx* ctx, uint64_t out[8])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    out[0] = ctx->mapper ? ctx->mapper->decoy_distinct() : 0;
    out[1] = ctx->mapper ? ctx->mapper->decoy_slots() : 0;
    std::lock_guard<std::mutex> g(ctx->filter_mu);
    const Mapper::DecoyOutcome& t = ctx->sample.filter_counts.decoy;
    out[2] = t.reads_judged; out[3] = t.bases_judged; out[4] = t.reads_dropped; out[5] = t.bases_dropped; out[6] = t.valid; out[7] = t.hits;
    API_END(ctx)
}

int drprg_hip_decoy_lookup(drprg_hip_ctx* ctx, const uint64_t* kmers, uint64_t n, uint8_t* found)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!ctx->read_filter.decoy()) throw Error(DRPRG_EINVAL, "decoy screen: no decoy set is loaded (drprg_hip_set_decoy)");
    if (n && (!kmers || !found)) throw Error(DRPRG_EINVAL, "null argument");
    std::vector<uint64_t> canon(n);
    for (uint64_t i = 0; i < n; ++i) canon[i] = dev::dc_canonical(kmers[i], ctx->read_filter.decoy_k);
    m.decoy_lookup(canon, found);
    API_END(ctx)
}

int drprg_hip_decoy_screen_device(drprg_hip_ctx* ctx, const void* d_text, const void* d_words, const void* d_npos, uint64_t n_npos, const void* d_offsets,
    uint64_t n_reads, uint64_t n_bases, void* d_valid, void* d_hits, void* d_flags, uint64_t out[4], void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    if (d_text && d_words) throw Error(DRPRG_EINVAL, "decoy screen: the bases come as text or as packed words, not both");
    uint64_t res[5];
    m.decoy_screen_device(ctx->read_filter, (const uint8_t*)d_text, (const uint32_t*)d_words, (const uint64_t*)d_npos, n_npos, (const uint64_t*)d_offsets, n_reads,
        n_bases, (uint32_t*)d_valid, (uint32_t*)d_hits, (uint8_t*)d_flags, res, (hipStream_t)hip_stream);
    for (int i = 0; i < 4; ++i) out[i] = res[i];
    if (res[4]) throw Error(DRPRG_EINVAL, "decoy screen: the offsets do not ascend from 0 to n_bases");
    API_END(ctx)
}

// ---- the resident sample -----------------------------------------------------------------------------------------------------
} // extern "C"

bool drprg::reads_resident(drprg_hip_ctx* ctx, const char* path)
{
    const std::vector<Mapper*> all = mappers_of(ctx);
    if (all.empty()) return false;
    for (Mapper* m : all)
        if (!m->kept_complete()) return false;
    const std::vector<std::string>& mapped = ctx->sample.mapped_paths;
    return !path || (mapped.size() == 1 && mapped[0] == path);
}

extern "C" {

int drprg_hip_keep_reads(drprg_hip_ctx* ctx, uint64_t max_bytes)
{
    API_BEGIN(ctx)
    need_mapper(ctx);
    for (Mapper* m : mappers_of(ctx)) m->keep_reads(max_bytes);
    // (reads mapped before this call are not resident: only a context that has mapped nothing yet can stand for a file)
    if (ctx->sample.total_bases != 0) ctx->sample.mapped_paths.assign(2, std::string());
    API_END(ctx)
}

int drprg_hip_map_resident(drprg_hip_ctx* ctx, drprg_hip_ctx* from)
{
    API_BEGIN(ctx)
    if (!from || from == ctx) throw Error(DRPRG_EINVAL, "drprg_hip_map_resident needs another open context");
    need_mapper(ctx);
    const std::vector<Mapper*> dst = mappers_of(ctx), src = mappers_of(from);
    if (!reads_resident(from, nullptr)) throw Error(DRPRG_ENODATA, "the other context does not hold all of its reads in device memory");
    if (dst.size() != src.size()) throw Error(DRPRG_EINVAL, "the two contexts span different numbers of devices");
    for (size_t i = 0; i < dst.size(); ++i)
        if (dst[i]->device() != src[i]->device()) throw Error(DRPRG_EINVAL, "the two contexts list different devices");
    ctx->sample.host_coverage_valid = false;
    for (size_t i = 0; i < dst.size(); ++i) ctx->sample.accepted_reads += dst[i]->map_kept_from(*src[i]); // (what `from` accepted under ITS cap: exactly those reads)
    ctx->sample.total_bases += from->sample.total_bases;
    ctx->sample.mapped_paths.insert(ctx->sample.mapped_paths.end(), from->sample.mapped_paths.begin(), from->sample.mapped_paths.end());
    reduce_devices(ctx);
    API_END(ctx)
}

int drprg_hip_resident_info(drprg_hip_ctx* ctx, uint64_t out[4])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    out[0] = reads_resident(ctx, nullptr) ? 1 : 0;
    out[1] = out[2] = 0;
    for (Mapper* m : mappers_of(ctx)) {
        out[1] += m->kept_bytes();
        out[2] += m->kept().size();
    }
    out[3] = ctx->last_discover_resident ? 1 : 0;
    API_END(ctx)
}

// ---- subsample and dedup: two selections among the resident reads, recorded alike ---------------------------------------------
// (each of the two shared refusals stands between refusals of the entry's own, in the order they have always been made)
static void refuse_several_devices(const drprg_hip_ctx* ctx, const std::string& entry)
{
    if (!ctx->extra.empty()) throw Error(DRPRG_EINVAL, entry + ": a context over several devices is not served");
}

static void refuse_unordered(const drprg_hip_ctx* ctx, const Mapper& m, const std::string& entry)
{
    if (ctx->sample.fastx_unordered && m.kept_complete()) // (a sample that is not resident is refused for that, by the mapper)
        throw Error(DRPRG_EINVAL, entry + ": drprg_hip_map_fastx handed this sample's blocks over in no particular order, so its reads have no "
                                          "file-order numbers (drprg_hip_set_ordered_ingest(ctx, 1) before the file is mapped)");
}

// what a selection did: into the entry's four outputs, its record, and the context
static void record_selection(drprg_hip_ctx* ctx, Selection& sel, const Mapper::SubsampleResult& r, std::vector<uint8_t>& flags, uint64_t out[4])
{
    out[0] = r.reads_before; out[1] = r.bases_before; out[2] = r.reads_kept; out[3] = r.bases_kept;
    sel.done = true;
    sel.reads_before = r.reads_before;
    for (int i = 0; i < 4; ++i) sel.counts[i] = out[i];
    sel.flags = std::move(flags);
    if (r.reads_kept != r.reads_before) { // the context now stands for the kept reads alone
        ctx->sample.host_coverage_valid = false;
        ctx->sample.total_bases = r.bases_kept;
        ctx->sample.accepted_reads = r.reads_kept;
    }
}

// the keep flags of the last `entry` call, one byte per read of the sample before it
static void copy_selection_flags(const Selection& sel, const std::string& entry, uint8_t* flags, uint64_t n)
{
    if (!sel.done) throw Error(DRPRG_EINVAL, entry + "_flags: no " + entry + " call since the last reset");
    if (n != sel.reads_before) throw Error(DRPRG_EINVAL, entry + "_flags: the sample held " + std::to_string(sel.reads_before) + " reads, not " + std::to_string(n));
    if (n && !flags) throw Error(DRPRG_EINVAL, "null output");
    if (n == 0) return; // (`flags` may be null)
    if (sel.flags.empty()) std::memset(flags, 1, n);
    else std::memcpy(flags, sel.flags.data(), n);
}

int drprg_hip_subsample(drprg_hip_ctx* ctx, uint64_t target_bases, uint64_t seed, uint64_t out[4])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    Mapper& m = need_mapper(ctx);
    refuse_several_devices(ctx, "drprg_hip_subsample");
    if (ctx->max_covg < 0xFFFFFFFFull)
        throw Error(DRPRG_EINVAL, "drprg_hip_subsample: a depth cap is set (drprg_hip_set_max_covg); the prefix cap and the random subsample are alternatives");
    refuse_unordered(ctx, m, "drprg_hip_subsample");
    std::vector<uint8_t> flags;
    const Mapper::SubsampleResult r = m.subsample_kept(target_bases, seed, flags);
    record_selection(ctx, ctx->sample.subsample, r, flags, out);
    API_END(ctx)
}

int drprg_hip_subsample_flags(drprg_hip_ctx* ctx, uint8_t* flags, uint64_t n)
{
    API_BEGIN(ctx)
    copy_selection_flags(ctx->sample.subsample, "drprg_hip_subsample", flags, n);
    API_END(ctx)
}

int drprg_hip_dedup(drprg_hip_ctx* ctx, uint32_t key_bits, uint64_t out[4])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    Mapper& m = need_mapper(ctx);
    if (key_bits < 1 || key_bits > 64) throw Error(DRPRG_EINVAL, "drprg_hip_dedup: key_bits must be 1..64");
    refuse_several_devices(ctx, "drprg_hip_dedup");
    refuse_unordered(ctx, m, "drprg_hip_dedup");
    std::vector<uint8_t> flags;
    const Mapper::SubsampleResult r = m.dedup_kept(key_bits, flags);
    record_selection(ctx, ctx->sample.dedup, r, flags, out);
    API_END(ctx)
}

int drprg_hip_dedup_flags(drprg_hip_ctx* ctx, uint8_t* flags, uint64_t n)
{
    API_BEGIN(ctx)
    copy_selection_flags(ctx->sample.dedup, "drprg_hip_dedup", flags, n);
    API_END(ctx)
}

int drprg_hip_dedup_keys_device(drprg_hip_ctx* ctx, const void* d_words, const void* d_offsets, uint64_t n_reads, uint64_t n_bases, const void* d_npos, uint64_t n_npos,
    void* d_keys, void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    m.dedup_keys_device((const uint32_t*)d_words, (const uint64_t*)d_offsets, n_reads, n_bases, (const uint64_t*)d_npos, n_npos, (unsigned long long*)d_keys,
        (hipStream_t)hip_stream);
    API_END(ctx)
}

// ---- mate overlap (the rule: include/drprg_hip.h "mate overlap") -----------------------------------------------------------------
int drprg_hip_set_pair_overlap(drprg_hip_ctx* ctx, uint32_t min_overlap, uint32_t error_milli, int clip)
{
    API_BEGIN(ctx)
    if (min_overlap == 0 && error_milli == 0 && !clip) {
        ctx->pair = Mapper::PairSetting {};
        for (Mapper* m : mappers_of(ctx)) m->pair_record(false);
        ctx->dedup_pairs = false; // (duplicate pairs: without mates there are no pairs)
        for (Mapper* m : mappers_of(ctx)) m->pair_dedup_record(false);
        return DRPRG_OK;
    }
    if (min_overlap < 8 || min_overlap > dev::PO_MAX_LEN) throw Error(DRPRG_EINVAL, "mate overlap: the smallest overlap is a whole number in 8 .. 1024");
    if (error_milli > 250) throw Error(DRPRG_EINVAL, "mate overlap: the share of differing columns is at most 0.25 (250 thousandths)");
    if (clip && ctx->pair.merge) throw Error(DRPRG_EINVAL, "mate overlap: mate merging is on (drprg_hip_set_pair_merge), and merging subsumes the clip");
    ctx->pair = Mapper::PairSetting { min_overlap, error_milli, clip != 0, ctx->pair.merge };
    for (Mapper* m : mappers_of(ctx)) m->pair_record(true); // (from the next block on the resident set numbers its reads by side)
    API_END(ctx)
}

int drprg_hip_begin_mates(drprg_hip_ctx* ctx)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!ctx->pair.on()) throw Error(DRPRG_EINVAL, "drprg_hip_begin_mates: no mate-overlap setting (drprg_hip_set_pair_overlap)");
    refuse_several_devices(ctx, "drprg_hip_begin_mates");
    m.begin_mates();
    ctx->sample.mates_begun = true;
    API_END(ctx)
}

int drprg_hip_pair_overlap(drprg_hip_ctx* ctx, uint64_t out[12])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    Mapper& m = need_mapper(ctx);
    if (!ctx->pair.on()) throw Error(DRPRG_EINVAL, "drprg_hip_pair_overlap: no mate-overlap setting (drprg_hip_set_pair_overlap)");
    refuse_several_devices(ctx, "drprg_hip_pair_overlap");
    if (ctx->max_covg < 0xFFFFFFFFull)
        throw Error(DRPRG_EINVAL, "drprg_hip_pair_overlap: a depth cap is set (drprg_hip_set_max_covg); the prefix cap would take side 1 alone, and a pair "
                                  "needs both of its mates");
    refuse_unordered(ctx, m, "drprg_hip_pair_overlap");
    std::vector<int32_t> shifts;
    uint64_t counts[dev::PO_WORDS], merged[dev::PM_WORDS];
    m.pair_overlap_kept(ctx->pair, shifts, counts, ctx->pair.merge ? merged : nullptr);
    SampleState& s = ctx->sample;
    s.pair_done = true;
    s.pair_shifts = std::move(shifts);
    for (int i = 0; i < dev::PO_WORDS; ++i) out[i] = s.pair_counts[i] = counts[i];
    s.pair_merge_done = ctx->pair.merge;
    for (int i = 0; i < dev::PM_WORDS; ++i) s.pair_merge_counts[i] = ctx->pair.merge ? merged[i] : 0;
    if (counts[dev::PO_BASES_KEPT] != counts[dev::PO_BASES_BEFORE]) { // the context now stands for the cut reads
        s.host_coverage_valid = false;
        s.total_bases = counts[dev::PO_BASES_KEPT];
    }
    API_END(ctx)
}

int drprg_hip_pair_overlap_shifts(drprg_hip_ctx* ctx, int32_t* d, uint64_t n)
{
    API_BEGIN(ctx)
    const SampleState& s = ctx->sample;
    if (!s.pair_done) throw Error(DRPRG_EINVAL, "drprg_hip_pair_overlap_shifts: no drprg_hip_pair_overlap call since the last reset");
    if (n != s.pair_shifts.size())
        throw Error(DRPRG_EINVAL, "drprg_hip_pair_overlap_shifts: the sample held " + std::to_string(s.pair_shifts.size()) + " pairs, not " + std::to_string(n));
    if (n && !d) throw Error(DRPRG_EINVAL, "null output");
    if (n) std::memcpy(d, s.pair_shifts.data(), n * sizeof(int32_t));
    API_END(ctx)
}

int drprg_hip_pair_overlap_info(drprg_hip_ctx* ctx, uint64_t out[12])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    for (int i = 0; i < 12; ++i) out[i] = ctx->sample.pair_counts[i]; // (all zero before the stage has run)
    API_END(ctx)
}

int drprg_hip_pair_overlap_device(drprg_hip_ctx* ctx, const void* d_words_a, const void* d_offsets_a, uint64_t n_bases_a, const void* d_npos_a, uint64_t n_npos_a,
    const void* d_words_b, const void* d_offsets_b, uint64_t n_bases_b, const void* d_npos_b, uint64_t n_npos_b, uint64_t n_pairs, void* d_shift, void* d_keep_a,
    void* d_keep_b, uint64_t out[12], void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    static_assert(dev::PO_WORDS == 12, "drprg_hip_pair_overlap_device writes twelve counts");
    const Mapper::PairSide a { (const uint32_t*)d_words_a, (const uint64_t*)d_offsets_a, n_bases_a, (const uint64_t*)d_npos_a, n_npos_a };
    const Mapper::PairSide b { (const uint32_t*)d_words_b, (const uint64_t*)d_offsets_b, n_bases_b, (const uint64_t*)d_npos_b, n_npos_b };
    m.pair_overlap_device(ctx->pair, a, b, n_pairs, (int32_t*)d_shift, (uint64_t*)d_keep_a, (uint64_t*)d_keep_b, out, (hipStream_t)hip_stream);
    API_END(ctx)
}

// ---- mate merging (the rule: include/drprg_hip.h "mate merging") -------------------------------------------------------------------
int drprg_hip_set_pair_merge(drprg_hip_ctx* ctx, int on)
{
    API_BEGIN(ctx)
    if (on && !ctx->pair.on()) throw Error(DRPRG_EINVAL, "drprg_hip_set_pair_merge: no mate-overlap setting (drprg_hip_set_pair_overlap): without mates there is nothing to merge");
    if (on && ctx->pair.clip) throw Error(DRPRG_EINVAL, "drprg_hip_set_pair_merge: the mate-overlap setting clips, and merging subsumes the clip");
    ctx->pair.merge = on != 0;
    API_END(ctx)
}

int drprg_hip_pair_merge_info(drprg_hip_ctx* ctx, uint64_t out[8])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    static_assert(dev::PM_WORDS == 8, "drprg_hip_pair_merge_info writes eight counts");
    for (int i = 0; i < 8; ++i) out[i] = ctx->sample.pair_merge_counts[i]; // (all zero before the stage has merged)
    API_END(ctx)
}

int drprg_hip_pair_merge_device(drprg_hip_ctx* ctx, const void* d_words_a, const void* d_offsets_a, uint64_t n_bases_a, const void* d_npos_a, uint64_t n_npos_a,
    const void* d_words_b, const void* d_offsets_b, uint64_t n_bases_b, const void* d_npos_b, uint64_t n_npos_b, uint64_t n_pairs, void* d_shift, void* d_out_offsets,
    void* d_out_words, uint64_t cap_words, void* d_out_npos, uint64_t cap_npos, uint64_t* n_out_npos, uint64_t out12[12], uint64_t out8[8], void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out12 || !out8 || !n_out_npos) throw Error(DRPRG_EINVAL, "null output");
    const Mapper::PairSide a { (const uint32_t*)d_words_a, (const uint64_t*)d_offsets_a, n_bases_a, (const uint64_t*)d_npos_a, n_npos_a };
    const Mapper::PairSide b { (const uint32_t*)d_words_b, (const uint64_t*)d_offsets_b, n_bases_b, (const uint64_t*)d_npos_b, n_npos_b };
    m.pair_merge_device(ctx->pair, a, b, n_pairs, (int32_t*)d_shift, (uint64_t*)d_out_offsets, (uint32_t*)d_out_words, cap_words, (uint64_t*)d_out_npos, cap_npos,
        n_out_npos, out12, out8, (hipStream_t)hip_stream);
    API_END(ctx)
}

// ---- duplicate pairs (the rule: include/drprg_hip.h "duplicate pairs") --------------------------------------------------------------
int drprg_hip_set_dedup_pairs(drprg_hip_ctx* ctx, int on)
{
    API_BEGIN(ctx)
    if (on && !ctx->pair.on()) throw Error(DRPRG_EINVAL, "drprg_hip_set_dedup_pairs: no mate-overlap setting (drprg_hip_set_pair_overlap): without mates there are no pairs");
    ctx->dedup_pairs = on != 0;
    for (Mapper* m : mappers_of(ctx)) m->pair_dedup_record(on != 0);
    API_END(ctx)
}

int drprg_hip_dedup_pairs(drprg_hip_ctx* ctx, uint32_t key_bits, uint64_t out[8])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    Mapper& m = need_mapper(ctx);
    if (key_bits < 1 || key_bits > 64) throw Error(DRPRG_EINVAL, "drprg_hip_dedup_pairs: key_bits must be 1..64");
    refuse_several_devices(ctx, "drprg_hip_dedup_pairs");
    if (!ctx->dedup_pairs) throw Error(DRPRG_EINVAL, "drprg_hip_dedup_pairs: the stage is not switched on (drprg_hip_set_dedup_pairs, before drprg_hip_pair_overlap)");
    if (m.kept_complete() && !ctx->sample.pair_done)
        throw Error(DRPRG_EINVAL, "drprg_hip_dedup_pairs: no drprg_hip_pair_overlap call on this sample: its reads are not paired");
    refuse_unordered(ctx, m, "drprg_hip_dedup_pairs");
    std::vector<uint8_t> flags;
    uint64_t counts[8], levels[32];
    const Mapper::SubsampleResult r = m.dedup_pairs_kept(key_bits, flags, counts, levels);
    SampleState& s = ctx->sample;
    uint64_t four[4];
    record_selection(ctx, s.pair_dedup, r, flags, four);
    for (int i = 0; i < 8; ++i) out[i] = s.pair_dedup_words[i] = counts[i];
    for (int i = 0; i < 32; ++i) s.pair_dedup_words[8 + i] = levels[i];
    API_END(ctx)
}

int drprg_hip_dedup_pairs_flags(drprg_hip_ctx* ctx, uint8_t* flags, uint64_t n)
{
    API_BEGIN(ctx)
    copy_selection_flags(ctx->sample.pair_dedup, "drprg_hip_dedup_pairs", flags, n);
    API_END(ctx)
}

int drprg_hip_dedup_pairs_info(drprg_hip_ctx* ctx, uint64_t out[40])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    for (int i = 0; i < 40; ++i) out[i] = ctx->sample.pair_dedup_words[i]; // (all zero before the stage has run)
    API_END(ctx)
}

int drprg_hip_dedup_pairs_device(drprg_hip_ctx* ctx, const void* d_words_a, const void* d_offsets_a, uint64_t n_bases_a, const void* d_npos_a, uint64_t n_npos_a,
    const void* d_words_b, const void* d_offsets_b, uint64_t n_bases_b, const void* d_npos_b, uint64_t n_npos_b, uint64_t n_pairs, uint32_t key_bits, void* d_keys,
    void* d_keep, void* d_copies, uint64_t out[40], void* hip_stream)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    static_assert(dev::PD_WORDS == 40, "drprg_hip_dedup_pairs_device writes forty words");
    const Mapper::PairSide a { (const uint32_t*)d_words_a, (const uint64_t*)d_offsets_a, n_bases_a, (const uint64_t*)d_npos_a, n_npos_a };
    const Mapper::PairSide b { (const uint32_t*)d_words_b, (const uint64_t*)d_offsets_b, n_bases_b, (const uint64_t*)d_npos_b, n_npos_b };
    m.dedup_pairs_device(a, b, n_pairs, key_bits, (uint64_t*)d_keys, (uint8_t*)d_keep, (uint32_t*)d_copies, out, (hipStream_t)hip_stream);
    API_END(ctx)
}

int drprg_hip_select_reads(drprg_hip_ctx* ctx, const uint64_t* anchors, uint64_t n_anchors, uint32_t A, uint64_t window_bytes, uint8_t* bases,
    uint64_t bases_cap, uint64_t* offsets, uint64_t* ids, uint64_t reads_cap, uint64_t out[2])
{
    API_BEGIN(ctx)
    if (!out || (n_anchors && !anchors)) throw Error(DRPRG_EINVAL, "null argument");
    if (A == 0 || A > 31) throw Error(DRPRG_EINVAL, "anchor length must be 1..31");
    if (!reads_resident(ctx, nullptr)) throw Error(DRPRG_ENODATA, "not every read of the sample is resident");
    const std::vector<uint64_t> kmers(anchors, anchors + n_anchors);
    std::vector<uint8_t> sel_bases;
    std::vector<uint64_t> sel_offsets(1, 0), sel_ids;
    uint64_t first_block = 0; // (ids count the kept blocks through all the mappers, like drprg_hip_resident_info)
    for (Mapper* m : mappers_of(ctx)) {
        const size_t had = sel_ids.size();
        m->select_reads_with_anchors(kmers, A, sel_bases, sel_offsets, &sel_ids, window_bytes);
        for (size_t i = had; i < sel_ids.size(); ++i) sel_ids[i] += first_block << 32;
        first_block += m->kept().size();
    }
    out[0] = sel_ids.size();
    out[1] = sel_bases.size();
    if (sel_ids.size() > reads_cap || sel_bases.size() > bases_cap) throw Error(DRPRG_EOVERFLOW, "the selected reads do not fit the caller's buffers");
    if ((!sel_bases.empty() && !bases) || !offsets || (!sel_ids.empty() && !ids)) throw Error(DRPRG_EINVAL, "null output buffer");
    if (!sel_bases.empty()) std::memcpy(bases, sel_bases.data(), sel_bases.size());
    std::memcpy(offsets, sel_offsets.data(), sel_offsets.size() * sizeof(uint64_t));
    if (!sel_ids.empty()) std::memcpy(ids, sel_ids.data(), sel_ids.size() * sizeof(uint64_t));
    API_END(ctx)
}

} // extern "C"
