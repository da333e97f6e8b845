// capi_genotype.cpp -- behind the coverage vector: genotype, discover, update-PRG, and the coverage cache between them.
#include "capi_ctx.h"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <set>

using namespace drprg;

// the sample's coverage as it stands, genotyped
static GenotypeResult genotype_sample(drprg_hip_ctx* ctx, const char* vcf_refs)
{
    sync_host_coverage(ctx);
    const SampleState& s = ctx->sample;
    return genotype(ctx->index, s.covg, s.prg_reads, s.total_bases, ctx->params, vcf_refs ? vcf_refs : "");
}

static void write_candidate_regions(const std::string& dir, const GenotypeResult& r)
{
    std::ofstream o(dir + "/candidate_regions.tsv");
    o << "#locus\tstart\tend\tlow_start\tlow_end\tmax_covg\tconsensus\n";
    for (const CandidateRegion& c : r.candidates)
        o << c.chrom << "\t" << c.start << "\t" << c.end << "\t" << c.low_start << "\t" << c.low_end << "\t" << c.max_covg << "\t" << c.seq << "\n";
    if (!o) throw Error(DRPRG_EIO, "cannot write " + dir + "/candidate_regions.tsv");
}

// the PRGs of an update, written; the variants that found no place in them, said
static void write_prgs(const char* out_prg, const std::vector<std::pair<std::string, std::string>>& prgs, const std::vector<std::string>& skipped)
{
    for (const std::string& s : skipped) std::fprintf(stderr, "drprg-hip: novel variant at %s could not be placed in the PRG\n", s.c_str());
    std::ofstream o(out_prg);
    for (auto& p : prgs) o << ">" << p.first << "\n" << p.second << "\n";
    if (!o) throw Error(DRPRG_EIO, std::string("cannot write ") + out_prg);
}

extern "C" {

int drprg_hip_genotype(drprg_hip_ctx* ctx, const char* vcf_refs, const char* out_vcf, const char* sample)
{
    API_BEGIN(ctx)
    if (!out_vcf) throw Error(DRPRG_EINVAL, "null output path");
    GenotypeResult r = genotype_sample(ctx, vcf_refs);
    write_vcf(out_vcf, r, sample && *sample ? sample : "sample");
    ctx->ginfo[0] = r.exp_depth_covg; ctx->ginfo[1] = r.min_kmer_covg; ctx->ginfo[2] = (uint32_t)r.present.size(); ctx->ginfo[3] = (uint32_t)r.records.size();
    ctx->last_model = r.model;
    ctx->last_dropped = r.dropped_low_coverage.size();
    ctx->last_records = std::move(r.records);
    API_END(ctx)
}

// ---- discover (SURVEY.md section 8f NEXT-2) ---------------------------------------------------------------
int drprg_hip_discover(drprg_hip_ctx* ctx, const char* vcf_refs, const char* out_dir, const char* sample, uint32_t* n_candidates)
{
    API_BEGIN(ctx)
    if (!out_dir) throw Error(DRPRG_EINVAL, "null output directory");
    GenotypeResult r = genotype_sample(ctx, vcf_refs);
    const std::string dir = out_dir, smp = sample && *sample ? sample : "sample";
    write_candidate_regions(dir, r);
    {
        // pandora's denovo_paths.txt surface (/root/reference/src/lib.rs:648-697 parses "<N> loci with denovo variants" and the
        // line before every "<n> nodes" line).  Local assembly of the candidate regions is not implemented: no locus is ever
        // reported as carrying a novel variant, so MakePrg::update keeps the index PRG (/root/reference/src/lib.rs:299-301).
        std::ofstream o(dir + "/denovo_paths.txt");
        o << "1 samples\nSample " << smp << "\n0 loci with denovo variants\n";
        if (!o) throw Error(DRPRG_EIO, "cannot write " + dir + "/denovo_paths.txt");
        std::ofstream f(dir + "/denovo_sequences.fa");
    }
    if (n_candidates) *n_candidates = (uint32_t)r.candidates.size();
    API_END(ctx)
}

int drprg_hip_discover_reads(drprg_hip_ctx* ctx, const char* reads_path, const char* vcf_refs, const char* out_dir, const char* sample,
    int list_loci, uint32_t out[3])
{
    API_BEGIN(ctx)
    if (!out_dir || !reads_path) throw Error(DRPRG_EINVAL, "null argument");
    GenotypeResult r = genotype_sample(ctx, vcf_refs);
    const std::string dir = out_dir, smp = sample && *sample ? sample : "sample";
    write_candidate_regions(dir, r);
    // accurate reads (-I): whole strings between the anchors are counted; noisy reads: column-wise majority of their alignments
    DiscoverParams adp;
    if (!ctx->params.illumina) {
        adp.min_support = 4;
        adp.min_fraction = 0.6;
    }
    // the reads of this very file are in HBM (drprg_hip_keep_reads): the device picks the few that hold an anchor k-mer
    ResidentReads resident;
    // (a paired sample is two files: the resident reads stand for both, reads_path for side 1 alone)
    ctx->last_discover_resident = reads_resident(ctx, ctx->sample.mates_begun ? nullptr : reads_path);
    // (the pass over the file knows nothing of the read filter: rather than pile up reads the mapping never saw, say so)
    if (!ctx->last_discover_resident && ctx->sample.mates_begun)
        throw Error(DRPRG_ENODATA, "discover: the sample was mapped from two mate files (drprg_hip_begin_mates) and its reads are not resident in device memory; a "
                                   "pass over the file would pile up the first file's reads alone, uncut (raise DRPRG_HIP_KEEP_READS_GB)");
    if (!ctx->last_discover_resident && (ctx->sample.filter_counts.adapter.reads_cut || ctx->sample.filter_counts.front.reads_cut))
        throw Error(DRPRG_ENODATA, "discover: adapter trimming cut bases off reads of this sample and the cut reads are not resident in device memory; a pass "
                                   "over the file would pile up reads with their adapters (raise DRPRG_HIP_KEEP_READS_GB, or cut the file first)");
    if (!ctx->last_discover_resident && ctx->sample.filter_counts.trim.reads_lost_base)
        throw Error(DRPRG_ENODATA, "discover: read trimming cut bases off reads of this sample and the trimmed reads are not resident in device memory; a pass "
                                   "over the file would pile up untrimmed reads (raise DRPRG_HIP_KEEP_READS_GB, or trim the file first)");
    if (!ctx->last_discover_resident && ctx->sample.filter_counts.poly.reads_cut)
        throw Error(DRPRG_ENODATA, "discover: poly-tail trimming (--poly-tail) cut tails off reads of this sample and the cut reads are not resident in device memory; "
                                   "a pass over the file would pile up the reads with their tails (raise DRPRG_HIP_KEEP_READS_GB, or trim the file first)");
    if (!ctx->last_discover_resident && ctx->sample.filter_counts.cplx.reads_dropped)
        throw Error(DRPRG_ENODATA, "discover: the complexity filter (--min-complexity) dropped reads of this sample and the kept reads are not resident in device "
                                   "memory; a pass over the file would pile up the dropped reads too (raise DRPRG_HIP_KEEP_READS_GB, or filter the file first)");
    if (!ctx->last_discover_resident && ctx->sample.filter_counts.mask.reads_masked)
        throw Error(DRPRG_ENODATA, "discover: base masking (--mask-qual) made bases of this sample unknown and the masked reads are not resident in device memory; "
                                   "a pass over the file would pile up the bases as the file holds them (raise DRPRG_HIP_KEEP_READS_GB, or mask the file first)");
    if (!ctx->last_discover_resident && ctx->sample.filter_counts.decoy.reads_dropped)
        throw Error(DRPRG_ENODATA, "discover: the decoy screen dropped reads of this sample and the kept reads are not resident in device memory; a pass over "
                                   "the file would pile up the contaminant reads too (raise DRPRG_HIP_KEEP_READS_GB, or screen the file first)");
    if (!ctx->last_discover_resident && ctx->sample.filter_counts.reads_kept != ctx->sample.filter_counts.reads_seen)
        throw Error(DRPRG_ENODATA, "discover: the read filter dropped reads of this sample and the kept reads are not resident in device memory; a pass over "
                                   "the file would see the unfiltered reads (drprg_hip_keep_reads before drprg_hip_map_fastx; the executables take the limit "
                                   "from DRPRG_HIP_KEEP_READS_GB)");
    if (ctx->last_discover_resident)
        resident = [ctx](const std::vector<uint64_t>& anchors, uint32_t A, std::vector<uint8_t>& bases, std::vector<uint64_t>& offsets) {
            for (Mapper* m : mappers_of(ctx)) m->select_reads_with_anchors(anchors, A, bases, offsets);
        };
    // a depth cap that was reached: the file pass stops after the reads that were mapped (the resident ones are those already)
    // (only when every base of the running total came with its reads through this context: a total taken over with a coverage vector
    // says nothing about how many reads of the file stand behind it)
    const uint64_t max_reads = ctx->sample.cap_reached && !ctx->sample.bases_without_reads ? ctx->sample.accepted_reads : ~0ull;
    std::vector<NovelVariant> variants = assemble_candidate_regions(r, reads_path, ctx->threads, adp, ctx->params.illumina, resident, max_reads);
    write_denovo_paths(dir, smp, r, variants, list_loci != 0);
    if (out) {
        out[0] = (uint32_t)r.candidates.size();
        out[1] = (uint32_t)variants.size();
        std::set<std::string> loci;
        for (const NovelVariant& v : variants) loci.insert(v.chrom);
        out[2] = (uint32_t)loci.size();
    }
    ctx->last_discover = std::move(r);
    ctx->last_variants = std::move(variants);
    API_END(ctx)
}

int drprg_hip_update_prg(drprg_hip_ctx* ctx, const char* out_prg, uint32_t* n_applied)
{
    API_BEGIN(ctx)
    if (!out_prg) throw Error(DRPRG_EINVAL, "null output path");
    std::vector<std::pair<std::string, std::string>> prgs;
    for (const LocalGraph& g : ctx->index.prgs) prgs.emplace_back(g.name, g.prg);
    std::vector<std::string> skipped;
    const uint32_t n = update_prgs(prgs, ctx->last_discover, ctx->last_variants, &skipped);
    write_prgs(out_prg, prgs, skipped);
    if (n_applied) *n_applied = n;
    API_END(ctx)
}

int drprg_hip_update_prg_from_paths(drprg_hip_ctx* ctx, const char* denovo_paths, const char* out_prg, uint32_t* n_applied)
{
    API_BEGIN(ctx)
    if (!denovo_paths || !out_prg) throw Error(DRPRG_EINVAL, "null path");
    std::vector<std::pair<std::string, std::string>> prgs;
    std::vector<std::string> names;
    for (const LocalGraph& g : ctx->index.prgs) {
        prgs.emplace_back(g.name, g.prg);
        names.push_back(g.name);
    }
    GenotypeResult gr;
    std::vector<NovelVariant> variants;
    read_denovo_paths(denovo_paths, names, gr, variants);
    for (const LocusConsensus& lc : gr.consensus) // the node intervals must be this PRG's
        for (const ConsensusNode& n : lc.nodes)
            if (n.end > prgs[lc.prg].second.size() || prgs[lc.prg].second.compare(n.start, n.end - n.start, n.seq) != 0)
                throw Error(DRPRG_EINVAL, std::string(denovo_paths) + ": the nodes of " + lc.chrom + " are not intervals of this context's PRG");
    std::vector<std::string> skipped;
    const uint32_t n = update_prgs(prgs, gr, variants, &skipped);
    write_prgs(out_prg, prgs, skipped);
    if (n_applied) *n_applied = n;
    API_END(ctx)
}

// Coverage cache: `pandora discover` and the `pandora map` that follows stream the same reads against the same PRG
// (/root/reference/src/predict.rs:248-255, :296-302); the first saves its vector, the second takes it back if `tag` agrees.
static const char COVG_MAGIC[8] = { 'D', 'R', 'P', 'R', 'G', 'C', 'V', '1' };

int drprg_hip_save_coverage(drprg_hip_ctx* ctx, const char* path, const char* tag)
{
    API_BEGIN(ctx)
    if (!path || !tag) throw Error(DRPRG_EINVAL, "null argument");
    sync_host_coverage(ctx);
    std::ofstream o(path, std::ios::binary);
    const uint64_t hdr[4] = { std::strlen(tag), ctx->sample.covg.size(), ctx->sample.prg_reads.size(), ctx->sample.total_bases };
    uint64_t cnt[8] = { 0 };
    if (ctx->mapper) to_words(ctx->mapper->counters(), cnt);
    o.write(COVG_MAGIC, 8);
    o.write((const char*)hdr, sizeof hdr);
    o.write((const char*)cnt, sizeof cnt);
    o.write(tag, (std::streamsize)hdr[0]);
    o.write((const char*)ctx->sample.covg.data(), (std::streamsize)(ctx->sample.covg.size() * sizeof(uint32_t)));
    o.write((const char*)ctx->sample.prg_reads.data(), (std::streamsize)(ctx->sample.prg_reads.size() * sizeof(uint32_t)));
    if (!o) throw Error(DRPRG_EIO, std::string("cannot write ") + path);
    API_END(ctx)
}

int drprg_hip_load_coverage(drprg_hip_ctx* ctx, const char* path, const char* tag, uint64_t counters[8])
{
    API_BEGIN(ctx)
    if (!path || !tag) throw Error(DRPRG_EINVAL, "null argument");
    std::ifstream in(path, std::ios::binary);
    if (!in) return DRPRG_ENOENT;
    char magic[8];
    uint64_t hdr[4], cnt[8];
    in.read(magic, 8);
    in.read((char*)hdr, sizeof hdr);
    in.read((char*)cnt, sizeof cnt);
    if (!in || std::memcmp(magic, COVG_MAGIC, 8) != 0 || hdr[0] > (1u << 20)) return DRPRG_EFORMAT;
    std::string t(hdr[0], '\0');
    in.read(&t[0], (std::streamsize)hdr[0]);
    if (!in || t != tag || hdr[1] != 2 * (uint64_t)ctx->index.flat.total_knodes() || hdr[2] != ctx->index.prgs.size())
        return DRPRG_ENOENT; // another PRG / other reads / other parameters: not this run's vector
    std::vector<uint32_t> covg(hdr[1]), prg_reads(hdr[2]);
    in.read((char*)covg.data(), (std::streamsize)(covg.size() * sizeof(uint32_t)));
    in.read((char*)prg_reads.data(), (std::streamsize)(prg_reads.size() * sizeof(uint32_t)));
    if (!in) return DRPRG_EFORMAT;
    ctx->sample.covg.swap(covg);
    ctx->sample.prg_reads.swap(prg_reads);
    ctx->sample.host_coverage_valid = true;
    ctx->sample.total_bases = hdr[3];
    ctx->sample.bases_without_reads = true;
    if (ctx->mapper) ctx->mapper->upload(ctx->sample.covg, ctx->sample.prg_reads);
    if (counters) std::memcpy(counters, cnt, sizeof cnt);
    API_END(ctx)
}

int drprg_hip_genotype_alleles(drprg_hip_ctx* ctx, const char* out_tsv)
{
    API_BEGIN(ctx)
    if (!out_tsv) throw Error(DRPRG_EINVAL, "null output path");
    std::ofstream o(out_tsv);
    if (!o) throw Error(DRPRG_EIO, std::string("cannot write ") + out_tsv);
    o << "#chrom\tpos\tallele\tn_kmers\tglobal_kmer_nodes\n";
    for (const VcfRecord& rec : ctx->last_records)
        for (size_t a = 0; a < rec.allele_knodes.size(); ++a) {
            o << rec.chrom << "\t" << rec.pos << "\t" << a << "\t" << rec.allele_knodes[a].size() << "\t";
            for (size_t i = 0; i < rec.allele_knodes[a].size(); ++i) o << (i ? "," : "") << rec.allele_knodes[a][i];
            o << "\n";
        }
    if (!o) throw Error(DRPRG_EIO, std::string("short write to ") + out_tsv);
    API_END(ctx)
}

int drprg_hip_coverage_model(const drprg_hip_ctx* ctx, double out[12])
{
    if (!ctx || !out) return DRPRG_EINVAL;
    const CoverageModel& m = ctx->last_model;
    out[0] = m.exp_depth_covg; out[1] = m.bin ? 1 : 0; out[2] = m.e_rate; out[3] = m.nb_p; out[4] = m.nb_r; out[5] = m.branch;
    out[6] = m.mean; out[7] = m.var; out[8] = m.num_reads; out[9] = m.bin_p; out[10] = m.thresh; out[11] = (double)ctx->last_dropped;
    return DRPRG_OK;
}

int drprg_hip_genotype_info(const drprg_hip_ctx* ctx, uint32_t out[4])
{
    if (!ctx || !out) return DRPRG_EINVAL;
    std::memcpy(out, ctx->ginfo, sizeof ctx->ginfo);
    return DRPRG_OK;
}

} // extern "C"
