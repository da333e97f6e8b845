// switches.h -- the environment switches of the mapper's hot path, read and checked in one place (switches.cpp).  A Mapper reads them
// when it is constructed and again at reset_coverage; the launchers take what they need as parameters.  The index builder gets the tier
// switches from its caller (the context open, drprg_hip_index).  Malformed values are ignored: the built-in choice stays.
#pragma once
#include <cstddef>
#include <cstdint>
#include <optional>

namespace drprg {

// sketch_filter_kernel's chunk schedule (sketch_filter.hip make_filter_sched).  DRPRG_FT_SCHED=static | f,d,m[,a]: round 0's part of the
// tiles in 1/256, the divisor of the dynamic rounds x 16 (a round hands every wave 16 / d of an even share of what is left), the smallest
// chunk in tiles, and the fewest tiles per wave a batch must have for a dynamic schedule at all (64: below that the static split is as
// good, and cheaper)
struct FilterSchedKnobs {
    bool is_static = false;
    uint32_t f = 180, d = 32, m = 4, min_avg = 64;
};

// where the small tier's level-0 form tests its second stage (sketch_filter.hip): by the batch's format (the L2 block filter for packed
// batches, the LDS for ASCII ones), or DRPRG_FILTER_STAGE2=l2 | lds (any other value) whatever the format
enum class Stage2 { by_format, l2, lds };

// largest index (records) the middle tier serves: beyond it hashing every k-mer (sketch_wave_kernel) is faster -- measured crossover
// between 121 k records (2.5 against 3.7 ms per 10 M reads) and 244 k (5.4 against 4.2 ms)
constexpr size_t MID_MAX_RECORDS = 180000;

struct Switches {
    FilterSchedKnobs ft_sched;           // DRPRG_FT_SCHED
    uint32_t ft_grid = 0;                // DRPRG_FT_GRID=n: at most n workgroups of sketch_filter_kernel (0: no cap)
    bool ft_share_pinned = false;        // DRPRG_FT_SHARE=a,b,c,d (any scale) is set: these tile shares, no adaptation
    uint32_t ft_share[4] = { 256, 256, 256, 256 }; // ... summing to 1024 (even ones if the value is malformed)
    Stage2 stage2 = Stage2::by_format;   // DRPRG_FILTER_STAGE2
    bool direct_lds = false;             // DRPRG_DIRECT_FORM=lds: sketch_probe_kernel for every (k, w) of the direct sequence
    bool skip_read_cluster = false;      // DRPRG_FT_DEBUG bit 8: every read of the filtered sequence through the generic pipeline
    // read at open only: they shape construction
    std::optional<uint64_t> min_capacity;      // DRPRG_HIP_MIN_CAPACITY: smallest candidate / hit buffers, in entries
    bool force_mid_tier = false;               // DRPRG_FORCE_MID_TIER: k = 15 indexes take the middle tier however small
    size_t mid_max_records = MID_MAX_RECORDS;  // DRPRG_MID_MAX_RECORDS
};

Switches read_switches();

} // namespace drprg
