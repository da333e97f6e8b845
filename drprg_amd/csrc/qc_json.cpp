// qc_json.cpp -- the report of --qc-json (include/drprg_hip.h "read statistics"): the sample, the settings in force, the raw and the
// prepared snapshot, and the counters every preparation stage keeps.  Keys come in a fixed order; every count is written as the integer it
// is, means as decimals beside the sums they come from.  Host code only (read_stats_host.h).
#include "read_stats_host.h"
#include <cstdio>

namespace drprg {
namespace {

void put_string(std::string& o, const std::string& s)
{
    o += '"';
    for (const unsigned char c : s) {
        if (c == '"' || c == '\\') { o += '\\'; o += (char)c; }
        else if (c < 0x20) {
            char buf[8];
            std::snprintf(buf, sizeof buf, "\\u%04x", c);
            o += buf;
        } else o += (char)c;
    }
    o += '"';
}

void put_u64(std::string& o, uint64_t v) { o += std::to_string((unsigned long long)v); }

void put_ratio(std::string& o, uint64_t num, uint64_t den) // three decimals; 0 over nothing
{
    char buf[48];
    std::snprintf(buf, sizeof buf, "%.3f", den ? (double)num / (double)den : 0.0);
    o += buf;
}

void put_array(std::string& o, const uint64_t* v, size_t n, size_t stride = 1)
{
    o += '[';
    for (size_t i = 0; i < n; ++i) {
        if (i) o += ',';
        put_u64(o, v[i * stride]);
    }
    o += ']';
}

void put_snapshot(std::string& o, const uint64_t* w, bool with_qual)
{
    using namespace dev;
    uint64_t tot[RS_COLS];
    rs_base_totals(w, tot);
    o += "{\"reads\":"; put_u64(o, w[RS_READS]);
    o += ",\"bases\":"; put_u64(o, w[RS_BASES]);
    o += ",\"min_length\":"; put_u64(o, w[RS_MIN_LEN]);
    o += ",\"max_length\":"; put_u64(o, w[RS_MAX_LEN]);
    o += ",\"mean_length\":"; put_ratio(o, w[RS_BASES], w[RS_READS]);
    o += ",\"n50\":"; put_u64(o, rs_nx(w, 1, 2));
    o += ",\"n90\":"; put_u64(o, rs_nx(w, 9, 10));
    o += ",\"base_totals\":{";
    static const char* const cols[RS_COLS] = { "A", "C", "G", "T", "U" };
    for (uint32_t c = 0; c < RS_COLS; ++c) {
        if (c) o += ',';
        o += '"'; o += cols[c]; o += "\":";
        put_u64(o, tot[c]);
    }
    o += "},\"length_hist\":[";
    bool first = true;
    for (uint32_t b = 0; b < RS_LEN_BINS; ++b) {
        if (!w[RS_LEN_READS + b]) continue;
        if (!first) o += ',';
        first = false;
        o += '['; put_u64(o, rs_bin_low(b)); o += ','; put_u64(o, w[RS_LEN_READS + b]); o += ','; put_u64(o, w[RS_LEN_BASES + b]); o += ']';
    }
    o += ']';
    // per cycle: cut at the longest read, at most RS_CYCLES + 1 entries (the last one: every position from RS_CYCLES on)
    const size_t n_cyc = (size_t)(w[RS_MAX_LEN] < RS_CYCLES + 1 ? w[RS_MAX_LEN] : RS_CYCLES + 1);
    o += ",\"cycles\":{\"n\":"; put_u64(o, n_cyc);
    for (uint32_t c = 0; c < RS_COLS; ++c) {
        o += ",\""; o += cols[c]; o += "\":";
        put_array(o, w + RS_CYC_BASE + c, n_cyc, RS_COLS);
    }
    if (with_qual) {
        o += ",\"qual_sum\":"; put_array(o, w + RS_CYC_QSUM, n_cyc);
        o += ",\"mean_qual\":[";
        for (size_t p = 0; p < n_cyc; ++p) {
            uint64_t n = 0;
            for (uint32_t c = 0; c < RS_COLS; ++c) n += w[RS_CYC_BASE + p * RS_COLS + c];
            if (p) o += ',';
            put_ratio(o, w[RS_CYC_QSUM + p], n);
        }
        o += ']';
    }
    o += '}';
    if (with_qual) {
        uint64_t qsum = 0;
        for (uint32_t q = 0; q < RS_QUALS; ++q) qsum += q * w[RS_QUAL_HIST + q];
        o += ",\"mean_base_qual\":"; put_ratio(o, qsum, w[RS_BASES]);
        o += ",\"qual_hist\":"; put_array(o, w + RS_QUAL_HIST, RS_QUALS);
        o += ",\"readq_hist\":"; put_array(o, w + RS_READQ_HIST, RS_QUALS);
    }
    o += ",\"gc_hist\":"; put_array(o, w + RS_GC_HIST, RS_GC_BINS);
    o += '}';
}

} // namespace

std::string qc_json(const QcReport& r)
{
    std::string o;
    o += "{\"sample\":"; put_string(o, r.sample);
    o += ",\"format\":\"drprg-hip read statistics 1\"";
    o += ",\"length_resolution\":\"exact below 1024, 1/64 above\"";
    o += ",\"qualities\":"; o += r.with_qual ? "true" : "false";
    o += ",\"prepared_is_raw\":"; o += r.prepared_is_raw ? "true" : "false";
    o += ",\"prepared_lies\":\"behind trimming, adapters, poly tails, masking, the read filter, the complexity test, the decoy screen and the depth cap; in front of dedup and subsample\"";
    o += ",\"settings\":{";
    for (size_t i = 0; i < r.settings.size(); ++i) {
        if (i) o += ',';
        put_string(o, r.settings[i].first); o += ':'; put_u64(o, r.settings[i].second);
    }
    o += "},\"raw\":";
    put_snapshot(o, r.raw, r.with_qual);
    o += ",\"prepared\":";
    put_snapshot(o, r.prepared ? r.prepared : r.raw, r.with_qual);
    o += ",\"stages\":{";
    for (size_t i = 0; i < r.stages.size(); ++i) {
        if (i) o += ',';
        put_string(o, r.stages[i].first); o += ':';
        put_array(o, r.stages[i].second.data(), r.stages[i].second.size());
    }
    o += "}}\n";
    return o;
}

} // namespace drprg
