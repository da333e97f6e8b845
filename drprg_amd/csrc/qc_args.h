// qc_args.h -- --qc-json FILE and --qc-no-qual as both executables take them (include/drprg_hip.h "read statistics").
#pragma once
#include "../../include/drprg_hip.h"
#include "read_stats_host.h"
#include <cstdio>
#include <string>
#include <vector>

namespace drprg {

struct QcArgs {
    std::string json; // --qc-json FILE: empty = not set
    bool no_qual = false; // --qc-no-qual
    bool any() const { return !json.empty(); }
    int mode() const { return json.empty() ? 0 : no_qual ? 2 : 1; } // drprg_hip_set_read_stats
    // what is wrong with the two together (a usage error: exit 2)
    std::string check() const
    {
        if (no_qual && json.empty()) return "--qc-no-qual belongs to --qc-json";
        return std::string();
    }
    static const char* usage()
    {
        return "--qc-json FILE [--qc-no-qual]: the sample's read statistics, counted on the device as the reads arrive, written to FILE as JSON: reads, bases,\n"
               "              length histogram with N50 and N90, per-cycle base composition and quality, base and read quality histograms and GC, of\n"
               "              the reads as the file holds them (raw) and as they are handed to mapping (prepared: behind every --trim-*, --adapter,\n"
               "              --poly-tail, --mask-qual, --min/max-read-*, --min-complexity, --decoy and --max-covg; in front of --dedup and\n"
               "              --subsample-covg), with every stage's counters.  Statistics only: no verdict, no adapter guess (duplication\n"
               "              levels: --dedup-pairs; merged pairs: --pair-merge).  Needs qualities (FASTA is an error) unless --qc-no-qual leaves the three quality sections out.\n";
    }
    // -v: one line per snapshot, through `say` (a printf-like function of the executable with its own prefix)
    template <typename Say> void report(drprg_hip_ctx* ctx, Say&& say) const
    {
        std::vector<uint64_t> w(drprg_hip_read_stats_words());
        const bool same = drprg_hip_read_stats_prepared_is_raw(ctx) == 1;
        for (int which = 0; which < 2; ++which) {
            if (drprg_hip_read_stats_info(ctx, which, w.data(), w.size()) != 0) return;
            const uint64_t reads = w[dev::RS_READS], bases = w[dev::RS_BASES];
            uint64_t qsum = 0;
            for (uint32_t q = 0; q < dev::RS_QUALS; ++q) qsum += q * w[dev::RS_QUAL_HIST + q];
            char line[320], mq[48] = "";
            if (!no_qual) std::snprintf(mq, sizeof mq, " mean_base_qual=%.2f", bases ? (double)qsum / (double)bases : 0.0);
            std::snprintf(line, sizeof line, "read statistics: %s reads=%llu bases=%llu n50=%llu mean_length=%.1f%s%s", which ? "prepared" : "raw",
                (unsigned long long)reads, (unsigned long long)bases, (unsigned long long)rs_nx(w.data(), 1, 2), reads ? (double)bases / (double)reads : 0.0, mq,
                which && same ? " (prepared_is_raw)" : "");
            say(line);
        }
    }
};

} // namespace drprg
