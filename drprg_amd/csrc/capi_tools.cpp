// capi_tools.cpp -- entries that need no context: the post-VCF stage (annotate, report, BCF) and the ingest self-checks.
#include "../../include/drprg_hip.h"
#include "fastx.h"
#include "ingest.h"
#include "pgunzip.h"
#include "report.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <functional>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace drprg;

// FNV-1a of one read's bases: what both parse self-checks sum
static uint64_t fnv1a_read(const uint8_t* bases, uint64_t begin, uint64_t end)
{
    uint64_t h = 1469598103934665603ull;
    for (uint64_t j = begin; j < end; ++j) h = (h ^ bases[j]) * 1099511628211ull;
    return h;
}

// the entries below have no context: the error's text goes into the caller's buffer
static int report_guard(char* err, size_t err_len, const std::function<void()>& fn)
{
    auto put = [&](const char* m) {
        if (err && err_len) {
            std::strncpy(err, m, err_len - 1);
            err[err_len - 1] = 0;
        }
    };
    try {
        fn();
    } catch (const Error& e) {
        put(e.what());
        return e.code;
    } catch (const std::exception& e) {
        put(e.what());
        return DRPRG_EIO;
    }
    return DRPRG_OK;
}

extern "C" {

int drprg_hip_annotate(const char* index_dir, const char* pandora_vcf, const char* out_vcf, const drprg_hip_annotate_opts* o,
    char* err, size_t err_len)
{
    if (!index_dir || !pandora_vcf || !out_vcf || !o) return DRPRG_EINVAL;
    return report_guard(err, err_len, [&]() {
        report::AnnotateOpts a;
        a.filter.min_covg = o->min_covg; a.filter.max_covg = o->max_covg;
        a.filter.min_strand_bias = o->min_strand_bias; a.filter.min_gt_conf = o->min_gt_conf; a.filter.min_frs = o->min_frs;
        a.filter.has_max_indel = o->max_indel >= 0; a.filter.max_indel = o->max_indel;
        a.minor.maf = o->maf; a.minor.max_gaps = o->max_gaps; a.minor.max_called_gaps = o->max_called_gaps; a.minor.max_gaps_diff = o->max_gaps_diff;
        a.minor.minor_min_covg = o->minor_min_covg; a.minor.minor_min_strand_bias = o->minor_min_strand_bias;
        a.ignore_synonymous = o->ignore_synonymous != 0;
        a.id_seed = o->id_seed;
        report::annotate_vcf(report::IndexFiles { index_dir }, pandora_vcf, out_vcf, a);
    });
}

int drprg_hip_report_json(const char* index_dir, const char* annotated_vcf, const char* out_json, const char* sample, int padding,
    const char* index_version, char* err, size_t err_len)
{
    if (!index_dir || !annotated_vcf || !out_json) return DRPRG_EINVAL;
    return report_guard(err, err_len, [&]() {
        report::IndexFiles idx { index_dir };
        std::string version = index_version ? index_version : "";
        if (padding < 0 || !index_version) {
            report::IndexConfig c = report::read_config(idx.config());
            if (padding < 0) padding = c.padding;
            if (!index_version) version = c.version;
        }
        report::vcf_to_json(idx, annotated_vcf, out_json, sample ? sample : "sample", padding, version);
    });
}

} // extern "C"

// ---- ingest self-check (host only) ---------------------------------------------------------------------------
extern "C" int drprg_hip_vcf_to_bcf(const char* vcf_path, const char* bcf_path, char* err, size_t err_len)
{
    if (!vcf_path || !bcf_path) return DRPRG_EINVAL;
    return report_guard(err, err_len, [&]() { report::vcf_to_bcf(vcf_path, bcf_path); });
}

extern "C" int drprg_hip_gunzip_file(const char* gz_path, int threads, uint64_t chunk_bytes, const char* out_path, uint64_t out[3], char* err, size_t err_len)
{
    if (!gz_path || !out_path || !out) return DRPRG_EINVAL;
    return report_guard(err, err_len, [&]() {
        const int fd = open(gz_path, O_RDONLY);
        if (fd < 0) throw Error(DRPRG_ENOENT, std::string("cannot open ") + gz_path);
        struct stat sb;
        void* map = fstat(fd, &sb) == 0 && sb.st_size > 0 ? mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, fd, 0) : MAP_FAILED;
        close(fd);
        if (map == MAP_FAILED) throw Error(DRPRG_EIO, std::string("cannot map ") + gz_path);
        struct Unmap {
            void* p;
            size_t n;
            ~Unmap() { munmap(p, n); }
        } unmap { map, (size_t)sb.st_size };
        FILE* o = std::fopen(out_path, "wb");
        if (!o) throw Error(DRPRG_EIO, std::string("cannot write ") + out_path);
        struct Close {
            FILE* f;
            ~Close() { std::fclose(f); }
        } close_o { o };
        ParallelGunzip pg((const unsigned char*)map, (size_t)sb.st_size, threads, (size_t)chunk_bytes);
        std::vector<char> buf(size_t(8) << 20);
        uint64_t total = 0;
        for (size_t n; (n = pg.read(buf.data(), buf.size())) > 0; total += n)
            if (std::fwrite(buf.data(), 1, n, o) != n) throw Error(DRPRG_EIO, std::string("cannot write ") + out_path);
        out[0] = total;
        out[1] = pg.chunks_accepted();
        out[2] = pg.chunks_redone();
    });
}

extern "C" int drprg_hip_parse_fastx_ordered(const char* reads_path, int threads, uint64_t max_reads, uint64_t out[6], char* err, size_t err_len)
{
    if (!reads_path || !out) return DRPRG_EINVAL;
    return report_guard(err, err_len, [&]() {
        uint64_t sum = 0, n_reads = 0, n_bases = 0, batches = 0;
        IngestHooks hooks;
        hooks.submit_in_order = [&](const PinnedBatch& b) -> bool {
            const uint64_t n = std::min<uint64_t>(b.n_reads, max_reads - n_reads);
            for (uint64_t i = 0; i < n; ++i) sum += (n_reads + i + 1) * fnv1a_read(b.bases, b.offsets[i], b.offsets[i + 1]);
            n_reads += n;
            n_bases += b.offsets[n];
            ++batches;
            return n_reads < max_reads;
        };
        const IngestStats st = ingest_fastx(reads_path, threads, hooks);
        out[0] = n_reads; out[1] = n_bases; out[2] = sum; out[3] = batches; out[4] = (uint64_t)st.gz_mode; out[5] = st.discarded_reads;
    });
}

extern "C" int drprg_hip_parse_fastx(const char* reads_path, int threads, uint64_t out[5], char* err, size_t err_len)
{
    if (!reads_path || !out) return DRPRG_EINVAL;
    return report_guard(err, err_len, [&]() {
        uint64_t sum = 0, n_reads = 0, n_bases = 0, batches = 0;
        const bool no_digest = std::getenv("DRPRG_PARSE_NO_DIGEST") != nullptr; // (ingest timing without the checksum)
        auto digest = [&](const uint8_t* bases, const uint64_t* offsets, uint64_t n) {
            for (uint64_t i = 0; i < n && !no_digest; ++i) sum += fnv1a_read(bases, offsets[i], offsets[i + 1]); // (order-independent)
            n_reads += n;
            n_bases += offsets[n];
            ++batches;
        };
        // DRPRG_PARSE_FORMAT (self-check of the packing ingest, no device needed): "normalized" = the digest of the ASCII blocks with every
        // base upper-cased and every byte that is not ACGTacgt read as N; "packed" = the parser threads pack (IngestHooks::packed) and the
        // digest is taken over what the packed block says (letters back to A C G T, N at the positions in npos): the two must be equal
        const char* fmt = std::getenv("DRPRG_PARSE_FORMAT");
        const bool packed = fmt && std::string(fmt) == "packed", normalized = fmt && std::string(fmt) == "normalized";
        std::vector<uint8_t> tmp;
        auto digest_any = [&](const PinnedBatch& b) {
            if (!packed && !normalized) {
                digest(b.bases, b.offsets, b.n_reads);
                return;
            }
            tmp.resize(b.n_bases);
            if (b.packed) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(b.bases);
                for (uint64_t i = 0; i < b.n_bases; ++i) tmp[i] = (uint8_t)"ACTG"[(w[i >> 4] >> (2 * (i & 15))) & 3u];
                for (uint64_t i = 0; i < b.n_npos; ++i) {
                    if (b.npos[i] >= b.n_bases || (i && b.npos[i] <= b.npos[i - 1])) throw Error(DRPRG_EIO, "packed block: positions not ascending");
                    tmp[b.npos[i]] = 'N';
                }
            } else {
                for (uint64_t i = 0; i < b.n_bases; ++i) {
                    const uint8_t u = b.bases[i] & 0xDFu;
                    tmp[i] = (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? u : (uint8_t)'N';
                }
            }
            digest(tmp.data(), b.offsets, b.n_reads);
        };
        IngestHooks hooks;
        hooks.packed = packed;
        hooks.submit = digest_any;
        out[4] = 0;
        try {
            out[4] = (uint64_t)ingest_fastx(reads_path, threads, hooks).gz_mode;
        } catch (const Error& e) {
            if (e.code != DRPRG_EAGAIN_SERIAL) throw;
            FastxReader rd(reads_path);
            ReadBatch batch;
            while (rd.next_batch(batch, 1u << 20, 1ull << 28)) digest(batch.bases.data(), batch.offsets.data(), batch.n_reads());
        }
        out[0] = n_reads; out[1] = n_bases; out[2] = sum; out[3] = batches;
    });
}
