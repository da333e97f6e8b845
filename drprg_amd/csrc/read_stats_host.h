// read_stats_host.h -- what the host makes of a read-statistics snapshot (read_stats_words.h; include/drprg_hip.h "read statistics"): the
// Nx walk, the column sums, several devices' snapshots folded into one, and the report (qc_json.cpp).  No HIP header is needed: the
// library, both executables and a stand-alone sanitizer build (tools/read_stats_host_check.cpp) include it.
#pragma once
#include "read_stats_words.h"
#include <string>
#include <utility>
#include <vector>

namespace drprg {

// Nx of a snapshot: the bins walked downwards over len_bases until ceil(bases * num / den) bases are reached; the bin's lowest length
// (exact below 1024).  0 without a base.  N50: num / den = 1 / 2, N90: 9 / 10.
inline uint64_t rs_nx(const uint64_t* w, uint64_t num, uint64_t den)
{
    const unsigned __int128 total = w[dev::RS_BASES];
    if (total == 0) return 0;
    const unsigned __int128 need = (total * num + den - 1) / den;
    unsigned __int128 have = 0;
    for (uint32_t b = dev::RS_LEN_BINS; b-- > 0;) {
        have += w[dev::RS_LEN_BASES + b];
        if (have >= need) return dev::rs_bin_low(b);
    }
    return 0; // (a snapshot whose bins do not sum to its bases)
}

// the sample's base totals: the column sums of the per-cycle table (A, C, G, T, U)
inline void rs_base_totals(const uint64_t* w, uint64_t out[dev::RS_COLS])
{
    for (uint32_t c = 0; c < dev::RS_COLS; ++c) out[c] = 0;
    for (uint32_t p = 0; p <= dev::RS_CYCLES; ++p)
        for (uint32_t c = 0; c < dev::RS_COLS; ++c) out[c] += w[dev::RS_CYC_BASE + p * dev::RS_COLS + c];
}

// a += b, where both hold ~0 as the shortest read when they hold no read (Mapper::read_stats); rs_finish turns that into the reported 0
inline void rs_fold(uint64_t* a, const uint64_t* b)
{
    for (uint32_t i = 0; i < dev::RS_WORDS; ++i) {
        if (i == dev::RS_MIN_LEN) a[i] = b[i] < a[i] ? b[i] : a[i];
        else if (i == dev::RS_MAX_LEN) a[i] = b[i] > a[i] ? b[i] : a[i];
        else a[i] += b[i];
    }
}
inline void rs_finish(uint64_t* a)
{
    if (a[dev::RS_READS] == 0) a[dev::RS_MIN_LEN] = 0;
}

// The report --qc-json writes (qc_json.cpp).  settings / stages: name and numbers, in the order they are written; a snapshot: RS_WORDS words.
struct QcReport {
    std::string sample;
    bool with_qual = true, prepared_is_raw = true;
    std::vector<std::pair<std::string, uint64_t>> settings;
    const uint64_t* raw = nullptr;
    const uint64_t* prepared = nullptr;
    std::vector<std::pair<std::string, std::vector<uint64_t>>> stages;
};
std::string qc_json(const QcReport& r);

} // namespace drprg
