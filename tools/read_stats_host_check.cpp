// read_stats_host_check.cpp -- the host-side pieces of the read statistics (csrc/read_stats_words.h, read_stats_host.h, qc_json.cpp) in a
// stand-alone program, for a sanitizer build with the snapshot at its exact size:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/read_stats_host_check.cpp drprg_amd/csrc/qc_json.cpp -o /tmp/rs_check && /tmp/rs_check
// It walks the bin function over every length class, folds two snapshots, takes N50 / N90 and writes the report.  Exit 0: every check held.
#include "../drprg_amd/csrc/read_stats_host.h"
#include <cstdio>
#include <cstdlib>
#include <memory>

using namespace drprg;
using namespace drprg::dev;

static void need(bool ok, const char* what)
{
    if (ok) return;
    std::fprintf(stderr, "read_stats_host_check: %s\n", what);
    std::exit(1);
}

static void add_read(uint64_t* w, uint64_t L)
{
    const uint32_t b = rs_len_bin(L);
    need(b < RS_LEN_BINS, "a bin beyond the histogram");
    w[RS_READS] += 1;
    w[RS_BASES] += L;
    w[RS_LEN_READS + b] += 1;
    w[RS_LEN_BASES + b] += L;
    if (L < w[RS_MIN_LEN]) w[RS_MIN_LEN] = L;
    if (L > w[RS_MAX_LEN]) w[RS_MAX_LEN] = L;
    for (uint64_t p = 0; p < L && p < 2000; ++p) {
        const uint32_t c = (uint32_t)(p < RS_CYCLES ? p : RS_CYCLES);
        w[RS_CYC_BASE + c * RS_COLS + (uint32_t)(p % RS_COLS)] += 1;
        w[RS_CYC_QSUM + c] += 30;
        w[RS_QUAL_HIST + 30] += 1;
    }
    if (L) {
        w[RS_READQ_HIST + 30] += 1;
        w[RS_GC_HIST + 50] += 1;
    }
}

int main()
{
    // the bin function: monotone, its lowest length brackets L, the last bin is the last word of the histogram
    uint32_t last = 0;
    for (uint64_t L = 0; L < (1ull << 32); L += L < 70000 ? 1 : L / 997) {
        const uint32_t b = rs_len_bin(L);
        need(b >= last && b < RS_LEN_BINS, "the bin function is not monotone");
        need(rs_bin_low(b) <= L && (b + 1 == RS_LEN_BINS || L < rs_bin_low(b + 1)), "a length outside its bin");
        last = b;
    }
    need(rs_len_bin(0xFFFFFFFFull) == RS_LEN_BINS - 1, "the longest read is not in the last bin");
    // two snapshots at their exact size (heap: the sanitizer sees one word too many), folded
    std::unique_ptr<uint64_t[]> a(new uint64_t[RS_WORDS]()), b(new uint64_t[RS_WORDS]()), none(new uint64_t[RS_WORDS]());
    a[RS_MIN_LEN] = b[RS_MIN_LEN] = none[RS_MIN_LEN] = ~0ull;
    for (uint64_t L : { 1ull, 1ull, 2ull }) add_read(a.get(), L);
    need(rs_nx(a.get(), 1, 2) == 2 && rs_nx(a.get(), 9, 10) == 1, "N50 / N90 of {1, 1, 2}");
    for (uint64_t L : { 0ull, 150ull, 1023ull, 1024ull, 70000ull, 0xFFFFFFFFull }) add_read(b.get(), L);
    rs_fold(a.get(), b.get());
    rs_fold(a.get(), none.get());
    rs_finish(a.get());
    rs_finish(none.get());
    need(a[RS_READS] == 9 && a[RS_MIN_LEN] == 0 && a[RS_MAX_LEN] == 0xFFFFFFFFull && none[RS_MIN_LEN] == 0, "the fold");
    need(rs_nx(a.get(), 1, 2) == rs_bin_low(RS_LEN_BINS - 1) && rs_nx(none.get(), 1, 2) == 0, "N50 of the folded snapshot");
    uint64_t tot[RS_COLS];
    rs_base_totals(a.get(), tot);
    QcReport r;
    r.sample = "a \"sample\"\n\\";
    r.raw = a.get();
    r.prepared = none.get();
    r.prepared_is_raw = false;
    r.settings = { { "mask_qual", 10 }, { "max_covg", 0 } };
    r.stages = { { "read_trim", { 1, 2, 3, 4, 5, 6, 7, 8 } }, { "dedup", {} } };
    const std::string with = qc_json(r);
    r.with_qual = false;
    r.prepared = nullptr;
    const std::string without = qc_json(r);
    need(with.size() > without.size() && with.back() == '\n' && without.find("qual_hist") == std::string::npos && with.find("\"readq_hist\":[") != std::string::npos,
        "the report");
    std::printf("read_stats_host_check: ok (%zu and %zu bytes of JSON)\n", with.size(), without.size());
    return 0;
}
