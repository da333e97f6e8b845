// capi.cpp -- the C ABI declared in include/drprg_hip.h: contexts, errors, options, coverage and reset, the index and introspection entries,
// the thin wrappers around the host arithmetic.  The other subjects: capi_map.cpp, capi_prep.cpp, capi_reduce.cpp, capi_genotype.cpp, capi_tools.cpp.
#include "capi_ctx.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

using namespace drprg;

static thread_local std::string g_last_error;
static thread_local int g_open_error = DRPRG_OK; // why the last drprg_hip_open* of this thread returned NULL

int drprg::thread_error(int code, const std::string& what)
{
    g_last_error = what;
    return code;
}

// a drprg_hip_open* that returns NULL: why, for drprg_hip_last_error(NULL) and drprg_hip_open_error
static drprg_hip_ctx* open_failed(int code, const std::string& what)
{
    g_open_error = thread_error(code, what);
    return nullptr;
}

static void apply_defaults(MapParams& p, const drprg_hip_map_opts* o)
{
    p.illumina = o && o->illumina;
    p.error_rate = (o && o->error_rate > 0) ? o->error_rate : (p.illumina ? 0.001 : 0.11);
    p.max_diff = (o && o->max_diff > 0) ? o->max_diff : (p.illumina ? 2 * p.k + 1 : 250);
    p.min_cluster_size = o ? o->min_cluster_size : 10;
    p.genome_size = (o && o->genome_size) ? o->genome_size : 5000000;
    p.genotyping_error_rate = (o && o->genotyping_error_rate > 0) ? o->genotyping_error_rate : 0.01;
    p.kernel_mode = o ? o->kernel : 0;
    p.binomial = o && o->binomial;
}

void drprg::sync_host_coverage(drprg_hip_ctx* ctx)
{
    SampleState& s = ctx->sample;
    if (s.needs_reset) throw Error(DRPRG_EIO, "a reduce over the context's devices failed half way: drprg_hip_reset the context and map again");
    if (s.host_coverage_valid) return;
    if (ctx->mapper) {
        ctx->mapper->download(s.covg, s.prg_reads);
    } else {
        s.covg.assign(2 * (size_t)ctx->index.flat.total_knodes(), 0);
        s.prg_reads.assign(ctx->index.prgs.size(), 0);
    }
    s.host_coverage_valid = true;
}

extern "C" {

int drprg_hip_index(const char* prg_file, int w, int k, int threads)
{
    if (!prg_file) return DRPRG_EINVAL;
    try {
        PrgIndex::build_and_save(prg_file, w, k, threads > 0 ? threads : 1, read_switches());
    } catch (const Error& e) {
        return thread_error(e.code, e.what());
    } catch (const std::exception& e) {
        return thread_error(DRPRG_EIO, e.what());
    }
    return DRPRG_OK;
}

static drprg_hip_ctx* open_impl(const char* prg_file, int w, int k, int device, bool from_files, int threads, const int* more_devices = nullptr,
    int n_more = 0)
{
    g_open_error = DRPRG_OK;
    if (!prg_file) return open_failed(DRPRG_EINVAL, "null PRG path");
    std::unique_ptr<drprg_hip_ctx> ctx(new (std::nothrow) drprg_hip_ctx);
    if (!ctx) return open_failed(DRPRG_ENOMEM, "out of host memory");
    // the HIP runtime starts (first call of the process: 50-250 ms) while the index files are read
    std::thread warm;
    if (device >= 0) warm = std::thread(Mapper::warm_device, device);
    struct Join {
        std::thread& t;
        ~Join() { if (t.joinable()) t.join(); }
    } join_warm { warm };
    try {
        ctx->prg_file = prg_file;
        const Switches sw = read_switches(); // (the filter tier's; every Mapper reads its own)
        if (from_files) {
            // The k-mer graphs and the .idx beside the PRG are this build's own files.  An index directory made by the real
            // pandora holds files of the same names in pandora's private format: they are not parsed, the graphs are rebuilt
            // from the PRG string (tens of milliseconds for an mtb-sized panel), unless DRPRG_HIP_STRICT_INDEX is set.
            try {
                ctx->index.load(prg_file, w, k, sw);
            } catch (const Error& e) {
                const char* strict = std::getenv("DRPRG_HIP_STRICT_INDEX");
                if ((e.code != DRPRG_EFORMAT && e.code != DRPRG_ENOENT) || (strict && *strict && *strict != '0')) throw;
                std::fprintf(stderr, "drprg-hip: warning: %s; rebuilding the k-mer graphs from %s\n", e.what(), prg_file);
                ctx->index = PrgIndex();
                ctx->index.build(prg_file, w, k, threads > 0 ? threads : 1, sw);
            }
        } else ctx->index.build(prg_file, w, k, threads > 0 ? threads : 1, sw);
        ctx->params.w = w;
        ctx->params.k = k;
        apply_defaults(ctx->params, nullptr);
        if (warm.joinable()) warm.join();
        if (device >= 0) ctx->mapper.reset(new Mapper(ctx->index.flat, ctx->params, device));
        for (int i = 0; i < n_more; ++i) ctx->extra.emplace_back(new Mapper(ctx->index.flat, ctx->params, more_devices[i]));
    } catch (const Error& e) {
        return open_failed(e.code, e.what());
    } catch (const std::exception& e) {
        return open_failed(DRPRG_EIO, e.what());
    }
    return ctx.release();
}

drprg_hip_ctx* drprg_hip_open(const char* prg_file, int w, int k, int device) { return open_impl(prg_file, w, k, device, true, 1); }
drprg_hip_ctx* drprg_hip_open_prg(const char* prg_file, int w, int k, int device, int threads) { return open_impl(prg_file, w, k, device, false, threads); }

drprg_hip_ctx* drprg_hip_open_multi(const char* prg_file, int w, int k, const int* devices, int ndev, int from_files)
{
    if (!devices || ndev < 1) {
        g_last_error = "drprg_hip_open_multi needs at least one device";
        return nullptr;
    }
    for (int i = 0; i < ndev; ++i)
        if (devices[i] < 0) {
            g_last_error = "drprg_hip_open_multi: negative device id";
            return nullptr;
        }
    return open_impl(prg_file, w, k, devices[0], from_files != 0, 4, devices + 1, ndev - 1);
}

void drprg_hip_close(drprg_hip_ctx* ctx) { delete ctx; }

int drprg_hip_open_error(void) { return g_open_error; }

const char* drprg_hip_last_error(const drprg_hip_ctx* ctx) { return ctx ? ctx->last_error.c_str() : g_last_error.c_str(); }

int drprg_hip_set_opts(drprg_hip_ctx* ctx, const drprg_hip_map_opts* opts)
{
    API_BEGIN(ctx)
    apply_defaults(ctx->params, opts);
    if (ctx->mapper) ctx->mapper->set_params(ctx->params);
    for (auto& m : ctx->extra) m->set_params(ctx->params);
    API_END(ctx)
}

int drprg_hip_set_opts_sized(drprg_hip_ctx* ctx, const drprg_hip_map_opts* opts, size_t opts_size)
{
    static_assert(sizeof(drprg_hip_map_opts) == DRPRG_HIP_MAP_OPTS_SIZE, "drprg_hip_map_opts changed size: bump DRPRG_HIP_MAP_OPTS_SIZE");
    if (!ctx) return DRPRG_EINVAL;
    if (opts && opts_size != sizeof(drprg_hip_map_opts)) {
        ctx->last_error = "drprg_hip_map_opts: the caller's struct has " + std::to_string(opts_size) + " bytes, this library's "
            + std::to_string(sizeof(drprg_hip_map_opts)) + " (header / library mismatch)";
        return DRPRG_EINVAL;
    }
    return drprg_hip_set_opts(ctx, opts);
}

int drprg_hip_experimental(void) { return 0; } // (include/drprg_hip.h: one build of the library)

int drprg_hip_sync(drprg_hip_ctx* ctx)
{
    API_BEGIN(ctx)
    if (ctx->mapper) ctx->mapper->sync();
    API_END(ctx)
}

int drprg_hip_coverage_size(const drprg_hip_ctx* ctx, uint64_t* n_covg, uint64_t* n_prgs)
{
    if (!ctx) return DRPRG_EINVAL;
    if (n_covg) *n_covg = 2 * (uint64_t)ctx->index.flat.total_knodes();
    if (n_prgs) *n_prgs = ctx->index.prgs.size();
    return DRPRG_OK;
}

int drprg_hip_coverage(drprg_hip_ctx* ctx, uint32_t* covg, uint64_t n_covg, uint32_t* prg_reads, uint64_t n_prgs)
{
    API_BEGIN(ctx)
    sync_host_coverage(ctx);
    const SampleState& s = ctx->sample;
    if ((covg && n_covg != s.covg.size()) || (prg_reads && n_prgs != s.prg_reads.size())) throw Error(DRPRG_EINVAL, "coverage buffer size mismatch");
    if (covg) std::memcpy(covg, s.covg.data(), s.covg.size() * sizeof(uint32_t));
    if (prg_reads) std::memcpy(prg_reads, s.prg_reads.data(), s.prg_reads.size() * sizeof(uint32_t));
    API_END(ctx)
}

int drprg_hip_set_coverage(drprg_hip_ctx* ctx, const uint32_t* covg, uint64_t n_covg, const uint32_t* prg_reads, uint64_t n_prgs,
    uint64_t total_bases)
{
    API_BEGIN(ctx)
    if (!covg || !prg_reads || n_covg != 2 * (uint64_t)ctx->index.flat.total_knodes() || n_prgs != ctx->index.prgs.size())
        throw Error(DRPRG_EINVAL, "coverage buffer size mismatch");
    SampleState& s = ctx->sample;
    s.covg.assign(covg, covg + n_covg);
    s.prg_reads.assign(prg_reads, prg_reads + n_prgs);
    s.host_coverage_valid = true;
    s.total_bases = total_bases;
    s.bases_without_reads = true;
    if (ctx->mapper) ctx->mapper->upload(s.covg, s.prg_reads);
    API_END(ctx)
}

int drprg_hip_device_coverage(drprg_hip_ctx* ctx, void** d_covg, void** d_prg_reads)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    if (d_covg) *d_covg = m.d_covg();
    if (d_prg_reads) *d_prg_reads = m.d_prg_reads();
    API_END(ctx)
}

int drprg_hip_reset(drprg_hip_ctx* ctx)
{
    API_BEGIN(ctx)
    for (Mapper* m : mappers_of(ctx)) m->reset_coverage();
    ctx->sample = SampleState(); // (the settings stay: the depth cap, the read filter, trimming, the adapters)
    API_END(ctx)
}

int drprg_hip_counters(drprg_hip_ctx* ctx, uint64_t out[8])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null output");
    std::memset(out, 0, 8 * sizeof(uint64_t));
    if (ctx->mapper) {
        MapCounters c = ctx->mapper->counters();
        c += ctx->sample.extra_counts; // (the other devices of a multi-device context)
        to_words(c, out);
    }
    API_END(ctx)
}

int drprg_hip_estimate_parameters(const uint32_t* kmer_covg, uint64_t n, uint64_t clusters, uint64_t loci, uint32_t global_covg, int k, double e_rate,
    int bin, double out[10])
{
    if ((n && !kmer_covg) || !out) return DRPRG_EINVAL;
    const CoverageModel m = estimate_parameters(std::vector<uint32_t>(kmer_covg, kmer_covg + n), clusters, loci, global_covg, k, e_rate, bin != 0);
    out[0] = m.exp_depth_covg; out[1] = m.bin ? 1 : 0; out[2] = m.e_rate; out[3] = m.nb_p; out[4] = m.nb_r; out[5] = m.branch;
    out[6] = m.mean; out[7] = m.var; out[8] = m.num_reads; out[9] = m.bin_p;
    return DRPRG_OK;
}

int drprg_hip_kmer_log_prob(int use_bin, double nb_p, double nb_r, double bin_p, uint32_t fwd, uint32_t rev, uint32_t locus_reads, float* out)
{
    if (!out) return DRPRG_EINVAL;
    CoverageModel m;
    m.bin = use_bin != 0; m.nb_p = (float)nb_p; m.nb_r = (float)nb_r; m.bin_p = bin_p;
    *out = kmer_log_prob(m, fwd, rev, locus_reads);
    return DRPRG_OK;
}

int drprg_hip_prob_threshold(const float* logp, uint64_t n, int* out)
{
    if ((n && !logp) || !out) return DRPRG_EINVAL;
    *out = prob_threshold(std::vector<float>(logp, logp + n));
    return DRPRG_OK;
}

int drprg_hip_max_path(const drprg_hip_ctx* ctx, uint32_t prg, const float* logp, int thresh, uint32_t max_kmers_to_average, uint32_t* path,
    uint64_t cap, uint64_t* n_path)
{
    if (!ctx || !logp || !n_path || prg >= ctx->index.kgs.size()) return DRPRG_EINVAL;
    const KmerGraph& kg = ctx->index.kgs[prg];
    const std::vector<uint32_t> p = find_max_path(kg, std::vector<float>(logp, logp + kg.nodes.size()), thresh, max_kmers_to_average);
    *n_path = p.size();
    for (size_t i = 0; i < p.size() && i < cap; ++i) path[i] = p[i];
    return DRPRG_OK;
}

int drprg_hip_path_base_coverage(const drprg_hip_ctx* ctx, uint32_t prg, const uint32_t* path, uint64_t n_path, const uint32_t* covg2, uint32_t* out,
    uint64_t cap, uint64_t* n_out)
{
    if (!ctx || (n_path && !path) || !covg2 || !n_out || prg >= ctx->index.kgs.size()) return DRPRG_EINVAL;
    const KmerGraph& kg = ctx->index.kgs[prg];
    for (uint64_t i = 0; i < n_path; ++i)
        if (path[i] >= kg.nodes.size()) return DRPRG_EINVAL;
    const std::vector<uint32_t> b = base_coverage_along_path(ctx->index.prgs[prg], kg, std::vector<uint32_t>(path, path + n_path), covg2);
    *n_out = b.size();
    for (size_t i = 0; i < b.size() && i < cap; ++i) out[i] = b[i];
    return DRPRG_OK;
}

int drprg_hip_path_coverage_too_low(const uint32_t* base_covg, uint64_t n, uint32_t global_covg)
{
    if (n && !base_covg) return DRPRG_EINVAL;
    return path_coverage_too_low(std::vector<uint32_t>(base_covg, base_covg + n), global_covg) ? 1 : 0;
}

int drprg_hip_allele_stats(const uint32_t* fwd, const uint32_t* rev, uint32_t n, uint32_t min_kmer_covg, uint32_t out[6], double* gaps)
{
    if ((n && (!fwd || !rev)) || !out || !gaps) return DRPRG_EINVAL;
    const AlleleStats s = allele_stats(std::vector<uint32_t>(fwd, fwd + n), std::vector<uint32_t>(rev, rev + n), min_kmer_covg);
    out[0] = s.mean_fwd; out[1] = s.mean_rev; out[2] = s.med_fwd; out[3] = s.med_rev; out[4] = s.sum_fwd; out[5] = s.sum_rev;
    *gaps = s.gaps;
    return DRPRG_OK;
}

int drprg_hip_genotype_site(const uint32_t* mean_fwd, const uint32_t* mean_rev, const double* gaps, uint32_t n_alleles, double e,
    double eps, double* likelihood, int32_t* gt, double* gt_conf)
{
    if (!n_alleles || !mean_fwd || !mean_rev || !gaps || !likelihood || !gt || !gt_conf) return DRPRG_EINVAL;
    std::vector<AlleleStats> al(n_alleles);
    for (uint32_t a = 0; a < n_alleles; ++a) {
        al[a].mean_fwd = mean_fwd[a]; al[a].mean_rev = mean_rev[a]; al[a].gaps = gaps[a];
    }
    int g = 0;
    genotype_site(al, e, eps, g, *gt_conf);
    *gt = g;
    for (uint32_t a = 0; a < n_alleles; ++a) likelihood[a] = al[a].likelihood;
    return DRPRG_OK;
}

int drprg_hip_filter_selfcheck(const drprg_hip_ctx* ctx, uint64_t out[8])
{
    if (!ctx || !out) return DRPRG_EINVAL;
    ctx->index.filter_selfcheck(out);
    return DRPRG_OK;
}

int drprg_hip_index_sizes(const drprg_hip_ctx* ctx, uint64_t sizes[5])
{
    if (!ctx || !sizes) return DRPRG_EINVAL;
    const FlatIndex& f = ctx->index.flat;
    sizes[0] = f.keys.size(); sizes[1] = f.rec_prg.size(); sizes[2] = ctx->index.prgs.size(); sizes[3] = f.total_knodes(); sizes[4] = f.slot_key.size();
    return DRPRG_OK;
}

int drprg_hip_index_export(const drprg_hip_ctx* ctx, uint64_t* keys, uint32_t* rec_off, uint32_t* rec_prg, uint32_t* rec_knode,
    uint8_t* rec_strand, uint32_t* prg_min_path_len, uint32_t* prg_knode_base)
{
    if (!ctx) return DRPRG_EINVAL;
    const FlatIndex& f = ctx->index.flat;
    if (keys) std::memcpy(keys, f.keys.data(), f.keys.size() * sizeof(uint64_t));
    if (rec_off) std::memcpy(rec_off, f.rec_off.data(), f.rec_off.size() * sizeof(uint32_t));
    if (rec_prg) std::memcpy(rec_prg, f.rec_prg.data(), f.rec_prg.size() * sizeof(uint32_t));
    if (rec_knode) std::memcpy(rec_knode, f.rec_knode_global.data(), f.rec_knode_global.size() * sizeof(uint32_t));
    if (rec_strand) std::memcpy(rec_strand, f.rec_strand.data(), f.rec_strand.size());
    if (prg_min_path_len) std::memcpy(prg_min_path_len, f.min_path_len.data(), f.min_path_len.size() * sizeof(uint32_t));
    if (prg_knode_base) std::memcpy(prg_knode_base, f.knode_base.data(), f.knode_base.size() * sizeof(uint32_t));
    return DRPRG_OK;
}

int drprg_hip_prg_nodes(const drprg_hip_ctx* ctx, uint32_t prg, uint32_t* starts, uint32_t* ends, uint32_t cap, uint32_t* n_nodes,
    uint32_t* n_sites)
{
    if (!ctx || prg >= ctx->index.prgs.size()) return DRPRG_EINVAL;
    const LocalGraph& g = ctx->index.prgs[prg];
    for (uint32_t i = 0; i < g.nodes.size() && i < cap; ++i) {
        if (starts) starts[i] = g.nodes[i].start;
        if (ends) ends[i] = g.nodes[i].end;
    }
    if (n_nodes) *n_nodes = (uint32_t)g.nodes.size();
    if (n_sites) *n_sites = (uint32_t)g.sites.size();
    return DRPRG_OK;
}

int drprg_hip_device_tables(drprg_hip_ctx* ctx, uint64_t out[6])
{
    API_BEGIN(ctx)
    need_mapper(ctx).device_tables(out);
    API_END(ctx)
}

int drprg_hip_kernel_timing(drprg_hip_ctx* ctx, int enable, int reset, double* ms_total, uint64_t* launches)
{
    API_BEGIN(ctx)
    Mapper& m = need_mapper(ctx);
    m.sync(); // (a batch in flight carries the events of the setting it was launched with)
    m.enable_kernel_timing(enable != 0);
    if (ms_total) *ms_total = m.sketch_ms_total();
    if (launches) *launches = m.sketch_launches();
    if (reset) m.reset_kernel_timing();
    API_END(ctx)
}

int drprg_hip_filter_schedule(drprg_hip_ctx* ctx, uint64_t out[20])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null pointer");
    need_mapper(ctx).filter_schedule(out);
    API_END(ctx)
}

int drprg_hip_buffer_info(drprg_hip_ctx* ctx, uint64_t out[6])
{
    API_BEGIN(ctx)
    if (!out) throw Error(DRPRG_EINVAL, "null pointer");
    need_mapper(ctx);
    std::memset(out, 0, 6 * sizeof(uint64_t));
    for (Mapper* m : mappers_of(ctx)) { // (several devices: the counts summed, the capacities the largest)
        uint64_t v[6];
        m->buffer_info(v);
        for (int i = 0; i < 3; ++i) out[i] += v[i];
        for (int i = 3; i < 5; ++i) out[i] = std::max(out[i], v[i]);
    }
    API_END(ctx)
}

} // extern "C"
