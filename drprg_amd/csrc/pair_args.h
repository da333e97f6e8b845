// pair_args.h -- --mate FILE, --pair-min-overlap O, --pair-error E and --pair-clip-overlap as both executables take them
// (include/drprg_hip.h "mate overlap"), --pair-merge beside them (include/drprg_hip.h "mate merging") and --dedup-pairs behind them
// (include/drprg_hip.h "duplicate pairs").
#pragma once
#include "../../include/drprg_hip.h"
#include <cstdio>
#include <cstdlib>
#include <string>

namespace drprg {

struct PairArgs {
    std::string mate; // --mate FILE: empty = not set
    uint32_t min_overlap = 30, error_milli = 50;
    bool clip = false, overlap_given = false, error_given = false;
    bool dedup_pairs = false; // --dedup-pairs
    bool merge = false;       // --pair-merge
    bool any() const { return !mate.empty(); }
    // each returns what is wrong with its value (a usage error: exit 2), or nothing
    std::string set_overlap(const char* v)
    {
        char* end = nullptr;
        const unsigned long long n = std::strtoull(v, &end, 10);
        if (end == v || *end || *v == '-' || *v == '+' || n < 8 || n > 1024) return std::string("--pair-min-overlap needs a whole number of bases in 8 .. 1024, not ") + v;
        min_overlap = (uint32_t)n;
        overlap_given = true;
        return std::string();
    }
    // a decimal in [0, 0.25] with at most three places, read digit by digit: no rounding of a binary fraction decides a threshold
    std::string set_error(const char* v)
    {
        const std::string bad = std::string("--pair-error needs a decimal in 0 .. 0.25 with at most three places, not ") + v;
        const char* p = v;
        unsigned long long whole = 0, milli = 0;
        int digits = 0, places = 0;
        for (; *p >= '0' && *p <= '9'; ++p, ++digits) whole = whole < 1000 ? whole * 10 + (unsigned)(*p - '0') : 1000;
        if (*p == '.')
            for (++p; *p >= '0' && *p <= '9'; ++p, ++digits, ++places) {
                if (places >= 3) return bad;
                milli = milli * 10 + (unsigned)(*p - '0');
            }
        if (*p || !digits) return bad;
        for (; places < 3; ++places) milli *= 10;
        milli += whole * 1000;
        if (milli > 250) return bad;
        error_milli = (uint32_t)milli;
        error_given = true;
        return std::string();
    }
    // what is wrong with the options together, max_covg being the depth cap the run would set (>= 4294967295: none)
    std::string check(uint64_t max_covg = ~0ull, bool dedup = false) const
    {
        if (mate.empty() && dedup_pairs) return "--dedup-pairs belongs to --mate: without the second mates there are no pairs (--dedup judges every read alone)";
        if (dedup_pairs && dedup)
            return "--dedup-pairs and --dedup are alternatives: --dedup would drop one mate of a pair and keep the other (give --dedup-pairs for paired reads)";
        if (mate.empty() && overlap_given) return "--pair-min-overlap belongs to --mate";
        if (mate.empty() && error_given) return "--pair-error belongs to --mate";
        if (mate.empty() && clip) return "--pair-clip-overlap belongs to --mate";
        if (mate.empty() && merge) return "--pair-merge belongs to --mate: without the second mates there is nothing to merge";
        if (merge && clip) return "--pair-merge and --pair-clip-overlap are alternatives: merging subsumes the clip";
        if (!mate.empty() && max_covg < 0xFFFFFFFFull)
            return "--mate and --max-covg are alternatives: the prefix cap would take the first file alone, and a pair needs both of its mates "
                   "(--subsample-covg cuts a paired sample to a depth)";
        return std::string();
    }
    int set_on(drprg_hip_ctx* ctx) const
    {
        if (!any()) return 0;
        if (int rc = drprg_hip_set_pair_overlap(ctx, min_overlap, error_milli, clip ? 1 : 0)) return rc;
        if (merge) // (off: the entry is never called)
            if (int rc = drprg_hip_set_pair_merge(ctx, 1)) return rc;
        return dedup_pairs ? drprg_hip_set_dedup_pairs(ctx, 1) : 0; // (off: the entry is never called)
    }
    static const char* usage()
    {
        return "--mate FILE [--pair-min-overlap O] [--pair-error E] [--pair-clip-overlap]: FILE holds the second mates of the reads of -i, in the same\n"
               "              order.  Both files are mapped and stay in device memory; then every pair is laid over itself (the second mate reverse-\n"
               "              complemented) at every shift, and the shift with the most columns in which both bases are known -- at least O, default\n"
               "              30, of which at most the share E differ, default 0.05 -- gives the insert: bases beyond it are adapter read-through and\n"
               "              are cut off both mates.  No adapter sequence is needed.  --pair-clip-overlap also cuts the second mate down to what\n"
               "              the first does not cover, so that every base of the molecule counts once.  A read whose mate an earlier stage dropped\n"
               "              passes unchanged.  Runs in front of --dedup and --subsample-covg; needs the reads resident (DRPRG_HIP_KEEP_READS_GB).\n"
               "  --pair-merge (beside --mate, instead of --pair-clip-overlap): every pair with such a shift becomes ONE read, the insert from the first\n"
               "              mate's first base to the second mate's last, in the first file's place; the second mate stays as a read of no bases.  Where\n"
               "              both mates read a column and disagree the base becomes unknown (N); a known base fills an unknown one.  No quality is used.\n"
               "  --dedup-pairs (beside --mate, instead of --dedup): behind the overlap stage and in front of --subsample-covg every pair whose two mates\n"
               "              are both identical to the mates of a pair before it in the files -- same lengths, same letters without case, unknown bases\n"
               "              at the same places; a mate that was dropped or emptied counts as no bases, so an orphan is judged against orphans -- is\n"
               "              dropped, both mates or neither, on the device.  Two fragments that merely start at the same base keep both their pairs,\n"
               "              where --dedup would drop the second one's first mate.  -v prints the duplication rate, --qc-json the duplication levels.\n"
               "              Forward orientation and exact identity only; no optical-distance rule.\n";
    }
    // -v: the twelve counts as one line, through `say`
    template <typename Say> static void report(const uint64_t c[12], Say&& say)
    {
        char line[512];
        std::snprintf(line, sizeof line, "mate overlap: pairs=%llu pairs_judged=%llu orphans=%llu pairs_too_long=%llu pairs_overlapping=%llu pairs_read_through=%llu "
                                         "bases_cut=%llu bases_clipped=%llu reads_emptied=%llu reads=%llu bases_before=%llu bases_kept=%llu",
            (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3], (unsigned long long)c[4], (unsigned long long)c[5],
            (unsigned long long)c[6], (unsigned long long)c[7], (unsigned long long)c[8], (unsigned long long)c[9], (unsigned long long)c[10], (unsigned long long)c[11]);
        say(line);
    }
    // -v: the eight counts of --pair-merge as one line, through `say`
    template <typename Say> static void report_merge(const uint64_t c[8], Say&& say)
    {
        char line[512];
        std::snprintf(line, sizeof line, "mate merging: pairs_merged=%llu columns_both=%llu columns_agreeing=%llu columns_disagreeing=%llu columns_filled=%llu "
                                         "columns_unknown=%llu bases_merged=%llu longest_merged=%llu",
            (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3], (unsigned long long)c[4], (unsigned long long)c[5],
            (unsigned long long)c[6], (unsigned long long)c[7]);
        say(line);
    }
    // -v: the eight counts of --dedup-pairs and the duplication rate as one line, through `say`
    template <typename Say> static void report_dedup(const uint64_t c[8], Say&& say)
    {
        char line[512];
        std::snprintf(line, sizeof line, "pair dedup: units=%llu units_with_bases=%llu units_both_mates=%llu units_dropped=%llu reads_before=%llu bases_before=%llu "
                                         "reads_kept=%llu bases_kept=%llu duplication_rate=%.6f",
            (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3], (unsigned long long)c[4], (unsigned long long)c[5],
            (unsigned long long)c[6], (unsigned long long)c[7], c[1] ? (double)c[3] / (double)c[1] : 0.0);
        say(line);
    }
};

} // namespace drprg
