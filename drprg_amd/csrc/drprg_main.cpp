// drprg_main.cpp -- `drprg predict` front end on top of the C ABI (include/drprg_hip.h).
//
// Mirrors the CLI surface of /root/reference/src/predict.rs:134-202 (+ Filterer src/filter.rs:165-197, MinorAllele
// src/minor.rs:19-49, global -v/-t src/cli.rs:81-93) and the sequence of Predict::run (src/predict.rs:204-317):
// validate index -> map on the GPU -> discover from that same pass (candidate regions; novel variants from a pile-up of the reads;
// PRG update + index + second mapping pass only if there are any) -> genotype
// -> pandora_genotyped.vcf -> <sample>.drprg.vcf -> <sample>.drprg.json.  Host orchestration is C++ here because
// the image has no Rust toolchain; a Rust drprg binds the same ABI.
#include "../../include/drprg_hip.h"
#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dirent.h>
#include <fstream>
#include <string>
#include <sys/stat.h>
#include <unistd.h>
#include <vector>
#include "adapter_args.h"
#include "decoy_args.h"
#include "mask_args.h"
#include "poly_args.h"
#include "pair_args.h"
#include "qc_args.h"

namespace {

[[noreturn]] void die(const std::string& m, int code = 1)
{
    std::fprintf(stderr, "drprg (hip): error: %s\n", m.c_str());
    std::exit(code);
}
bool exists(const std::string& p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0;
}
bool is_dir(const std::string& p)
{
    struct stat st;
    return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

// -x <path | species[@version]> (/root/reference/src/cli.rs:21-78); named indexes live in ~/.drprg/<species>/<species>-<version>
// *named: the index was found by species name, i.e. it is one `drprg index --download` fetched (/root/reference/src/index.rs:122):
// its k-mer graphs and .idx are the real pandora's files
std::string resolve_index(const std::string& s, bool* named = nullptr)
{
    if (named) *named = false;
    if (exists(s)) return s;
    if (named) *named = true;
    if (s.find('/') != std::string::npos) die("Received an index which is path-like but does not exist");
    std::string species = s, version = "latest";
    size_t at = s.find('@');
    if (at != std::string::npos) {
        species = s.substr(0, at);
        version = s.substr(at + 1);
    }
    const char* home = std::getenv("HOME");
    std::string base = std::string(home ? home : ".") + "/.drprg/" + species;
    if (!is_dir(base)) die("No index for species " + species + " found in " + std::string(home ? home : ".") + "/.drprg");
    if (version != "latest") {
        std::string p = base + "/" + species + "-" + version;
        if (!exists(p)) die("Version " + version + " does not exist for species " + species);
        return p;
    }
    std::vector<std::string> dirs;
    if (DIR* d = opendir(base.c_str())) {
        while (dirent* e = readdir(d))
            if (e->d_name[0] != '.' && is_dir(base + "/" + e->d_name)) dirs.push_back(base + "/" + e->d_name);
        closedir(d);
    }
    if (dirs.empty()) die("No index versions found in " + species + " directory " + base);
    std::string best = dirs[0];
    for (auto& d : dirs)
        if (d > best) best = d;
    return best;
}

// first dr.prg.k<K>.w<W>.idx in the index directory (find_prg_index_in, /root/reference/src/lib.rs:1222-1231)
bool find_prg_index(const std::string& dir, int& k, int& w)
{
    bool found = false;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            int kk, ww;
            char tail[8] = { 0 };
            if (std::sscanf(e->d_name, "dr.prg.k%d.w%d.%3s", &kk, &ww, tail) == 3 && std::strcmp(tail, "idx") == 0) {
                k = kk;
                w = ww;
                found = true;
                break;
            }
        }
        closedir(d);
    }
    return found;
}

std::string file_prefix(const std::string& path) // PathExt::prefix: file name up to the first '.'
{
    size_t s = path.find_last_of('/');
    std::string name = s == std::string::npos ? path : path.substr(s + 1);
    size_t dot = name.find('.', name.empty() || name[0] != '.' ? 0 : 1);
    return dot == std::string::npos ? name : name.substr(0, dot);
}

void usage()
{
    std::fprintf(stderr,
        "drprg predict -x <index dir | species[@version]> -i <reads.fq[.gz] | reads.bam> [-o DIR] [-s SAMPLE] [-I] [-S]\n"
        "              [-f MAF] [-d MIN_COVG] [-D MAX_COVG] [-b MIN_STRAND_BIAS] [-g MIN_GT_CONF] [-L MAX_INDEL] [-K MIN_FRS]\n"
        "              [-C MIN_CLUSTER_SIZE] [--debug] [-v] [-t THREADS] [--rebuild-index] [--subsample-covg D [--seed S]]\n"
        "              [--dedup] [--min-read-len L] [--max-read-len L] [--min-read-qual Q]\n"
        "              [--trim-front N] [--trim-tail N] [--trim-qual Q [--trim-window W]]\n"
        "              [--adapter SEQ]... [--adapter-error E] [--adapter-min-overlap O] [--adapter-indels] [--front-adapter SEQ]...\n"
        "              [--poly-tail LETTERS [--poly-min-len M]] [--min-complexity P] [--qc-json FILE [--qc-no-qual]]\n"
        "              [--mask-qual Q] [--decoy FASTA]... [--decoy-k K] [--decoy-min-frac F] [--decoy-min-kmers M]\n"
        "              [--mate FILE [--pair-min-overlap O] [--pair-error E] [--pair-clip-overlap | --pair-merge] [--dedup-pairs]]\n"
        "--poly-tail LETTERS (letters of ACGT, e.g. G or ACGT), --poly-min-len M (2 to 255, default 10): every read loses its longest suffix of\n"
        "              at least M bases that begins with one of the letters and holds at most min(n / 8, 5) other bases -- the tails two-colour\n"
        "              instruments (NextSeq, NovaSeq) leave when a cluster goes dark, which carry HIGH qualities.  On the device, behind --trim-*\n"
        "              and both --adapter sides, in front of everything else: the run is that of a file of the cut reads.  Needs no qualities.\n"
        "--min-complexity P (a whole percentage, 1 to 100; fastp's default is 30): a read is dropped when fewer than P %% of its neighbouring\n"
        "              base pairs differ (an unknown base differs from every letter) -- on the device, behind --trim-*, --adapter, --poly-tail,\n"
        "              --mask-qual and --min/max-read-*, in front of --decoy.  This build's own rules, after fastp.  Default: off.\n"
        "--mask-qual Q (a whole Phred value, 1 to 93): every base whose quality is below Q becomes an unknown base -- on the device, behind\n"
        "              --trim-* and --adapter and in front of everything else: the run is that of a file in which those bases are the letter N.\n"
        "              The read keeps its length, its place in the depth arithmetic and its mean quality; only the k-mers that hold a masked\n"
        "              base stop existing.  Needs qualities: FASTA, or a BAM record without them, is an error under it.  A threshold on what the\n"
        "              basecaller claims: at Nanopore qualities a Q of 10 or more leaves few 15-mers.  Default: off.\n"
        "--decoy FASTA (up to 8 times; plain or .gz), --decoy-k K (9 to 31, default 31), --decoy-min-frac F (in (0, 1], default 0.5),\n"
        "              --decoy-min-kmers M (default 1): a read is dropped as a contaminant when at least M of its k-mers, and at least the\n"
        "              fraction F of its k-mers without a letter other than ACGT, are k-mers of the decoy files in either orientation -- on\n"
        "              the device, behind --trim-*, --adapter and --min/max-read-*.  This build's own rule (k-mer containment, as bbduk\n"
        "              ref=); sized for mitochondrion, NTM genomes, phiX, not a human genome.\n"
        "--adapter SEQ (up to 4 times; 1 to 64 letters ACGT), --adapter-error E (0 to 0.5, default 0.1), --adapter-min-overlap O (default 3):\n"
        "              every read is cut at the leftmost start at which an adapter matches with at most floor(c * E) substitutions over the\n"
        "              c = min(adapter, rest of the read) letters compared, c >= O -- on the device, behind --trim-* and in front of\n"
        "              everything else.  Needs no qualities.\n"
        "--adapter-indels: an occurrence may carry insertions and deletions too (edit distance at most floor(m * E) over the whole adapter).\n"
        "--front-adapter SEQ (up to 4 times; needs --adapter-indels): 5' adapters, cut off the reads' starts behind the 3' cut.\n"
        "              Still missing: anchored adapters, pair overlap, indels inside an adapter that the read's end cuts short.\n"
        "--trim-front N, --trim-tail N, --trim-qual Q, --trim-window W: every read loses N bases at its start and N at its end and, under\n"
        "              --trim-qual (a decimal Phred value in (0, 93]), what lies outside its first and last window of W bases (1..32, default\n"
        "              4) whose MEAN PHRED VALUE is at least Q, then end bases below Q -- on the device, in front of the read filter and\n"
        "              everything else; --trim-qual needs qualities (FASTQ, or BAM records that hold them).\n"
        "--min-read-len L, --max-read-len L, --min-read-qual Q: reads shorter than L, longer than L or of a mean quality below Q (a decimal\n"
        "              Phred value; the mean of the error probabilities, as nanoq and chopper take it) are dropped on the device before\n"
        "              anything else sees them; --min-read-qual needs qualities (FASTQ, or BAM records that hold them).\n"
        "--subsample-covg D: the sample is cut at random to D x 4411532 bases on the device before discover and genotyping (reads in the\n"
        "              order of a 64-bit key made from the seed, default 1, and the read's number, up to and including the one that reaches\n"
        "              the target); needs the sample resident in device memory (DRPRG_HIP_KEEP_READS_GB, default 32), fails if it is not.\n"
        "--dedup: every read that is identical to a read before it in the file (same length, same bases case-insensitively, non-ACGT bases\n"
        "              at the same places; forward strand only) is dropped on the device, in front of --subsample-covg, discover and\n"
        "              genotyping; needs the sample resident in device memory (DRPRG_HIP_KEEP_READS_GB, default 32), fails if it is not.\n"
        "%s%s"
        "MI355X-native hot path; -p/-m/-M (external tools) are accepted and not needed: novel variants update the PRG in process.\n",
        drprg::PairArgs::usage(), drprg::QcArgs::usage());
}

} // namespace

// seconds since main() was entered, for the -v lines (where the wall time of a prediction goes); since the moment the parent
// process names in DRPRG_HIP_T0 (seconds since the epoch, e.g. `DRPRG_HIP_T0=$(date +%s.%N)`), when it does -- that adds the
// time the loader takes before main()
static double since_start()
{
    static const double t0 = [] {
        const char* e = std::getenv("DRPRG_HIP_T0");
        const double given = e ? std::atof(e) : 0;
        return given > 0 ? given : std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    }();
    return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count() - t0;
}

// 2-bit packed ingest (include/drprg_hip.h "packed reads") unless DRPRG_HIP_INPUT=ascii: a quarter of the bytes to page-lock, to move over
// PCIe and to keep in HBM; same results
static int packed_input()
{
    const char* e = std::getenv("DRPRG_HIP_INPUT");
    return !(e && std::string(e) == "ascii");
}

int main(int argc, char** argv)
{
    const double at_main = since_start();
    if (argc < 2 || std::strcmp(argv[1], "predict") != 0) {
        usage();
        return argc >= 2 && (!std::strcmp(argv[1], "-h") || !std::strcmp(argv[1], "--help")) ? 0 : 2;
    }
    std::string index, input, outdir = ".", sample;
    bool illumina = false, verbose = false, maf_given = false, rebuild_index = false;
    int threads = 1;
    bool subsample = false, seed_given = false, dedup = false;
    double subsample_covg = 0;
    uint64_t seed = 1;
    uint64_t min_read_len = 0, max_read_len = 0; // the read filter (include/drprg_hip.h "read filter"); 0 = not set
    uint32_t min_read_qual_milli = 0;
    uint64_t trim_front = 0, trim_tail = 0; // read trimming (include/drprg_hip.h "read trimming"); 0 = not set
    uint32_t trim_qual_milli = 0, trim_window = 0;
    uint32_t mask_qual = 0; // --mask-qual Q: base masking (include/drprg_hip.h "base masking"); 0 = not set
    drprg::AdapterArgs adapters; // --adapter SEQ, --adapter-error E, --adapter-min-overlap O (include/drprg_hip.h "adapter trimming")
    drprg::PairArgs pair; // --mate FILE, --pair-min-overlap O, --pair-error E, --pair-clip-overlap (include/drprg_hip.h "mate overlap")
    drprg::QcArgs qc; // --qc-json FILE, --qc-no-qual (include/drprg_hip.h "read statistics")
    drprg::PolyArgs poly; // --poly-tail LETTERS, --poly-min-len M, --min-complexity P (include/drprg_hip.h "poly tails", "read complexity")
    drprg::DecoyArgs decoy; // --decoy FASTA, --decoy-k K, --decoy-min-frac F, --decoy-min-kmers M (include/drprg_hip.h "decoy screen")
    uint32_t min_cluster = 10;
    drprg_hip_annotate_opts ao {};
    ao.min_covg = 3;
    ao.max_covg = INT_MAX;
    ao.min_strand_bias = 0.01f;
    ao.min_gt_conf = 0.0f;
    ao.min_frs = 0.0f;
    ao.max_indel = -1;
    ao.maf = 1.0f;
    ao.max_gaps = 0.5f;
    ao.max_called_gaps = 0.39f;
    ao.max_gaps_diff = 0.2f;
    ao.minor_min_covg = 3;
    ao.minor_min_strand_bias = 0.01f;
    auto need = [&](int& i) -> const char* {
        if (i + 1 >= argc) die(std::string("option ") + argv[i] + " needs a value", 2);
        return argv[++i];
    };
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-x" || a == "--index") index = need(i);
        else if (a == "-i" || a == "--input") input = need(i);
        else if (a == "-o" || a == "--outdir") outdir = need(i);
        else if (a == "-s" || a == "--sample") sample = need(i);
        else if (a == "-I" || a == "--illumina") illumina = true;
        else if (a == "-S" || a == "--ignore-synonymous") ao.ignore_synonymous = 1;
        else if (a == "-f" || a == "--maf") { ao.maf = std::strtof(need(i), nullptr); maf_given = true; }
        else if (a == "--max-gaps") ao.max_gaps = std::strtof(need(i), nullptr);
        else if (a == "--max-called-gaps") ao.max_called_gaps = std::strtof(need(i), nullptr);
        else if (a == "--max-gaps-diff") ao.max_gaps_diff = std::strtof(need(i), nullptr);
        else if (a == "--minor-min-covg") ao.minor_min_covg = std::atoi(need(i));
        else if (a == "--minor-min-strand-bias") ao.minor_min_strand_bias = std::strtof(need(i), nullptr);
        else if (a == "-d" || a == "--min-covg") ao.min_covg = std::atoi(need(i));
        else if (a == "-D" || a == "--max-covg") ao.max_covg = std::atoi(need(i));
        else if (a == "-b" || a == "--min-strand-bias") ao.min_strand_bias = std::strtof(need(i), nullptr);
        else if (a == "-g" || a == "--min-gt-conf") ao.min_gt_conf = std::strtof(need(i), nullptr);
        else if (a == "-L" || a == "--max-indel") ao.max_indel = std::atoi(need(i));
        else if (a == "-K" || a == "--min-frs") ao.min_frs = std::strtof(need(i), nullptr);
        else if (a == "-C" || a == "--pandora-min-cluster-size") min_cluster = (uint32_t)std::atoi(need(i));
        else if (a == "-p" || a == "--pandora" || a == "-m" || a == "--makeprg" || a == "-M" || a == "--mafft") (void)need(i);
        else if (a == "-t" || a == "--threads") threads = std::atoi(need(i));
        else if (a == "-v" || a == "--verbose") verbose = true;
        else if (a == "--debug") verbose = true;
        else if (a == "--rebuild-index") rebuild_index = true;
        else if (a == "--qc-json") qc.json = need(i);
        else if (a == "--qc-no-qual") qc.no_qual = true;
        else if (a == "--dedup") dedup = true;
        else if (a == "--mate") pair.mate = need(i);
        else if (a == "--pair-clip-overlap") pair.clip = true;
        else if (a == "--pair-merge") pair.merge = true;
        else if (a == "--dedup-pairs") pair.dedup_pairs = true;
        else if (a == "--pair-min-overlap") {
            const std::string e = pair.set_overlap(need(i));
            if (!e.empty()) die(e, 2);
        } else if (a == "--pair-error") {
            const std::string e = pair.set_error(need(i));
            if (!e.empty()) die(e, 2);
        }
        else if (a == "--subsample-covg") {
            char* end = nullptr;
            const char* v = need(i);
            subsample_covg = std::strtod(v, &end);
            if (end == v || *end || !(subsample_covg >= 0)) die(std::string("--subsample-covg needs a depth >= 0, not ") + v, 2);
            subsample = true;
        } else if (a == "--seed") { seed = std::strtoull(need(i), nullptr, 10); seed_given = true; }
        else if (a == "--min-read-len" || a == "--max-read-len") {
            char* end = nullptr;
            const char* v = need(i);
            const uint64_t n = std::strtoull(v, &end, 10);
            if (end == v || *end || *v == '-') die(a + " needs a number of bases, not " + v, 2);
            (a == "--min-read-len" ? min_read_len : max_read_len) = n;
        } else if (a == "--min-read-qual") {
            char* end = nullptr;
            const char* v = need(i);
            const double q = std::strtod(v, &end);
            if (end == v || *end || !(q >= 0) || q > 93) die(std::string("--min-read-qual needs a mean quality between 0 and 93, not ") + v, 2);
            min_read_qual_milli = (uint32_t)(q * 1000.0 + 0.5);
        }
        else if (a == "--trim-front" || a == "--trim-tail") {
            char* end = nullptr;
            const char* v = need(i);
            const uint64_t n = std::strtoull(v, &end, 10);
            if (end == v || *end || *v == '-') die(a + " needs a number of bases, not " + v, 2);
            (a == "--trim-front" ? trim_front : trim_tail) = n;
        } else if (a == "--trim-qual") {
            char* end = nullptr;
            const char* v = need(i);
            const double q = std::strtod(v, &end);
            if (end == v || *end || !(q > 0) || q > 93) die(std::string("--trim-qual needs a quality above 0 and at most 93, not ") + v, 2);
            trim_qual_milli = (uint32_t)(q * 1000.0 + 0.5);
            if (!trim_qual_milli) die(std::string("--trim-qual needs a quality of at least 0.001, not ") + v, 2);
        } else if (a == "--trim-window") {
            char* end = nullptr;
            const char* v = need(i);
            const uint64_t n = std::strtoull(v, &end, 10);
            if (end == v || *end || n < 1 || n > 32) die(std::string("--trim-window needs a window of 1 to 32 bases, not ") + v, 2);
            trim_window = (uint32_t)n;
        }
        else if (a == "--adapter") {
            const std::string e = adapters.add(need(i));
            if (!e.empty()) die(e, 2);
        } else if (a == "--front-adapter") {
            const std::string e = adapters.add_front(need(i));
            if (!e.empty()) die(e, 2);
        } else if (a == "--adapter-indels") adapters.indels = true;
        else if (a == "--adapter-error") {
            const std::string e = adapters.set_error(need(i));
            if (!e.empty()) die(e, 2);
        } else if (a == "--adapter-min-overlap") {
            const std::string e = adapters.set_overlap(need(i));
            if (!e.empty()) die(e, 2);
        }
        else if (a == "--mask-qual") {
            const std::string e = drprg::parse_mask_qual(need(i), mask_qual);
            if (!e.empty()) die(e, 2);
        }
        else if (a == "--poly-tail") {
            const std::string e = poly.set_letters(need(i));
            if (!e.empty()) die(e, 2);
        } else if (a == "--poly-min-len") {
            const std::string e = poly.set_min_len(need(i));
            if (!e.empty()) die(e, 2);
        } else if (a == "--min-complexity") {
            const std::string e = poly.set_complexity(need(i));
            if (!e.empty()) die(e, 2);
        }
        else if (a == "--decoy") {
            const std::string e = decoy.add(need(i));
            if (!e.empty()) die(e, 2);
        } else if (a == "--decoy-k") {
            const std::string e = decoy.set_k(need(i));
            if (!e.empty()) die(e, 2);
        } else if (a == "--decoy-min-frac") {
            const std::string e = decoy.set_frac(need(i));
            if (!e.empty()) die(e, 2);
        } else if (a == "--decoy-min-kmers") {
            const std::string e = decoy.set_kmers(need(i));
            if (!e.empty()) die(e, 2);
        }
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else die("unknown option " + a, 2);
    }
    if (seed_given && !subsample) die("--seed belongs to --subsample-covg", 2);
    if (max_read_len && max_read_len < min_read_len) die("--max-read-len is below --min-read-len: no read can pass", 2);
    if (trim_window && !trim_qual_milli) die("--trim-window belongs to --trim-qual", 2);
    if (const std::string e = adapters.check(); !e.empty()) die(e, 2);
    if (const std::string e = decoy.check(); !e.empty()) die(e, 2);
    if (const std::string e = poly.check(); !e.empty()) die(e, 2);
    if (const std::string e = qc.check(); !e.empty()) die(e, 2);
    if (const std::string e = pair.check(~0ull, dedup); !e.empty()) die(e, 2);
    if (index.empty() || input.empty()) {
        usage();
        return 2;
    }
    if (illumina && !maf_given) ao.maf = 0.1f; // default_value_if("is_illumina", .., "0.1"), src/minor.rs:26-33
    if (!exists(input)) die(input + " does not exist");
    if (pair.any() && !exists(pair.mate)) die(pair.mate + " does not exist");
    bool named_index = false;
    index = resolve_index(index, &named_index);
    // An index found by species name is a downloaded one: its dr.prg.k*.w*.idx and kmer_prgs/ are the real pandora's files.  If
    // they do not parse in the layout this build reads, rebuilding the graphs from dr.prg would run -- and silently hide that the
    // two programs may not agree on the k-mer graphs the coverage is counted on -- so that is an error here unless the user asks
    // for the rebuild (--rebuild-index / DRPRG_HIP_REBUILD_INDEX=1).  An index given as a path keeps the rebuild with a warning.
    {
        const char* rb = std::getenv("DRPRG_HIP_REBUILD_INDEX");
        if (named_index && !rebuild_index && !(rb && *rb && *rb != '0')) setenv("DRPRG_HIP_STRICT_INDEX", "1", 1);
    }
    if (mkdir(outdir.c_str(), 0777) != 0 && errno != EEXIST) die("Failed to create output directory " + outdir);
    // validate_index (/root/reference/src/predict.rs:400-418)
    int k = 0, w = 0;
    if (!find_prg_index(index, k, w)) die("Index is not valid due to missing file " + index + "/dr.prg.kX.wY.idx");
    for (const char* f : { "/.config.toml", "/dr.prg", "/kmer_prgs", "/panel.bcf", "/panel.bcf.csi", "/genes.fa", "/msas" })
        if (!exists(index + f)) die("Index is not valid due to missing file " + index + f);
    if (sample.empty()) sample = file_prefix(input);
    int device = 0;
    if (const char* d = std::getenv("DRPRG_HIP_DEVICE")) device = std::atoi(d);

    const std::string prg = index + "/dr.prg";
    // DRPRG_HIP_DEVICES=0,1,2,3: one context over several GPUs of the node (the reads shard by ingest block, the coverage
    // vectors are summed before the genotyping / report stages, which run once)
    std::vector<int> devices;
    if (const char* d = std::getenv("DRPRG_HIP_DEVICES"))
        for (const char* p = d; *p;) {
            char* end = nullptr;
            const long v = std::strtol(p, &end, 10);
            if (end == p) break;
            devices.push_back((int)v);
            p = *end ? end + 1 : end;
        }
    if (devices.size() == 1) device = devices[0];
    drprg_hip_ctx* ctx = devices.size() > 1 ? drprg_hip_open_multi(prg.c_str(), w, k, devices.data(), (int)devices.size(), 1)
                                            : drprg_hip_open(prg.c_str(), w, k, device);
    if (!ctx)
        die(std::string("cannot open the index: ") + drprg_hip_last_error(nullptr)
            + (named_index ? " (a downloaded index whose pandora files this build cannot read: --rebuild-index rebuilds the k-mer graphs from dr.prg)" : ""));
    drprg_hip_map_opts mo {};
    mo.illumina = illumina;
    mo.min_cluster_size = min_cluster;
    mo.genome_size = 4411532; // MTB_GENOME_SIZE, /root/reference/src/lib.rs:36
    if (int rc = drprg_hip_set_opts(ctx, &mo)) die(drprg_hip_last_error(ctx), -rc);
    drprg_hip_set_threads(ctx, threads);
    drprg_hip_set_input_format(ctx, packed_input()); // the parser threads pack the reads to 2 bits (DRPRG_HIP_INPUT=ascii: one byte per base)
    if (int rc = drprg_hip_set_read_filter(ctx, min_read_len, max_read_len, min_read_qual_milli)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_set_read_trim(ctx, trim_front, trim_tail, trim_qual_milli, trim_window)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_set_base_mask(ctx, mask_qual)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = poly.set_on(ctx, drprg_hip_set_poly_trim, drprg_hip_set_min_complexity)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_set_read_stats(ctx, qc.mode())) die(drprg_hip_last_error(ctx), -rc); // (this context alone: the report is the first mapping pass's)
    if (adapters.any())
        if (int rc = adapters.set_on(ctx, drprg_hip_set_adapters, drprg_hip_set_adapters2)) die(drprg_hip_last_error(ctx), -rc);
    if (decoy.any()) // (once per run: the second pass after a PRG update maps the resident reads, which are screened already)
        if (int rc = decoy.set_on(ctx, drprg_hip_set_decoy)) die(drprg_hip_last_error(ctx), -rc);
    // The reads stay in HBM after the mapping pass (up to DRPRG_HIP_KEEP_READS_GB per device, default 32, 0 = off): discover takes
    // the few reads it needs from there and a novel variant maps them again from there -- the file is read once.
    double keep_gb = 32;
    if (const char* e = std::getenv("DRPRG_HIP_KEEP_READS_GB")) keep_gb = std::atof(e);
    if (keep_gb > 0)
        if (int rc = drprg_hip_keep_reads(ctx, (uint64_t)(keep_gb * 1e9))) die(drprg_hip_last_error(ctx), -rc);
    if (subsample || dedup || pair.any()) drprg_hip_set_ordered_ingest(ctx, 1); // (all three number the reads in file order)
    if (pair.any() && !(keep_gb > 0)) die("--mate needs the reads resident in device memory: DRPRG_HIP_KEEP_READS_GB=0 switches that off");
    if (int rc = pair.set_on(ctx)) die(drprg_hip_last_error(ctx), -rc); // (this context alone: a second pass maps the resident reads, which are cut already)
    if (dedup && !(keep_gb > 0)) die("--dedup needs the reads resident in device memory: DRPRG_HIP_KEEP_READS_GB=0 switches that off");
    if (subsample && !(keep_gb > 0)) die("--subsample-covg needs the reads resident in device memory: DRPRG_HIP_KEEP_READS_GB=0 switches that off");
    if (verbose && std::getenv("DRPRG_HIP_T0")) std::fprintf(stderr, "[drprg-hip +%.3fs] main() entered\n", at_main);
    if (verbose) std::fprintf(stderr, "[drprg-hip +%.3fs] mapping %s against %s (k=%d w=%d) on device %d\n", since_start(), input.c_str(), index.c_str(), k, w, device);
    // discover + map share ONE pass over the reads (the reference runs two, /root/reference/src/predict.rs:248-302)
    if (int rc = drprg_hip_map_fastx(ctx, input.c_str())) die(drprg_hip_last_error(ctx), -rc);
    if (pair.any()) { // the second mates, in the same pass: side 2 of the sample
        if (int rc = drprg_hip_begin_mates(ctx)) die(std::string("--mate: ") + drprg_hip_last_error(ctx), -rc);
        if (int rc = drprg_hip_map_fastx(ctx, pair.mate.c_str())) die(drprg_hip_last_error(ctx), -rc);
    }
    if (verbose) std::fprintf(stderr, "[drprg-hip +%.3fs] reads mapped\n", since_start());
    if (verbose && (trim_front || trim_tail || trim_qual_milli)) {
        uint64_t ti[8] = {};
        if (drprg_hip_read_trim_info(ctx, ti) == 0)
            std::fprintf(stderr, "[drprg-hip +%.3fs] read trimming: reads_seen=%llu bases_seen=%llu reads_lost_base=%llu cut_front=%llu cut_tail=%llu "
                                 "qual_cut_front=%llu qual_cut_tail=%llu reads_emptied=%llu\n", since_start(), (unsigned long long)ti[0], (unsigned long long)ti[1],
                (unsigned long long)ti[2], (unsigned long long)ti[3], (unsigned long long)ti[4], (unsigned long long)ti[5], (unsigned long long)ti[6],
                (unsigned long long)ti[7]);
    }
    if (verbose && adapters.any()) {
        uint64_t ai[5] = {};
        if (!adapters.seqs.empty() && drprg_hip_adapter_trim_info(ctx, ai) == 0)
            std::fprintf(stderr, "[drprg-hip +%.3fs] adapter trimming: reads_seen=%llu bases_seen=%llu reads_cut=%llu bases_cut=%llu reads_emptied=%llu\n", since_start(),
                (unsigned long long)ai[0], (unsigned long long)ai[1], (unsigned long long)ai[2], (unsigned long long)ai[3], (unsigned long long)ai[4]);
        if (!adapters.front.empty() && drprg_hip_front_adapter_info(ctx, ai) == 0)
            std::fprintf(stderr, "[drprg-hip +%.3fs] front adapter trimming: reads_seen=%llu bases_seen=%llu reads_cut=%llu bases_cut=%llu reads_emptied=%llu\n", since_start(),
                (unsigned long long)ai[0], (unsigned long long)ai[1], (unsigned long long)ai[2], (unsigned long long)ai[3], (unsigned long long)ai[4]);
    }
    if (verbose && poly.tails()) { // (of the one pass over the file: a second pass after a PRG update maps the resident reads, which are cut already)
        uint64_t pt[5] = {};
        if (drprg_hip_poly_trim_info(ctx, pt) == 0)
            std::fprintf(stderr, "[drprg-hip +%.3fs] poly tail trimming: reads_seen=%llu bases_seen=%llu reads_cut=%llu bases_cut=%llu reads_emptied=%llu\n", since_start(),
                (unsigned long long)pt[0], (unsigned long long)pt[1], (unsigned long long)pt[2], (unsigned long long)pt[3], (unsigned long long)pt[4]);
    }
    if (verbose && mask_qual) { // (of the one pass over the file: a second pass after a PRG update maps the resident reads, which are masked already)
        uint64_t bm[5] = {};
        if (drprg_hip_base_mask_info(ctx, bm) == 0)
            std::fprintf(stderr, "[drprg-hip +%.3fs] base masking: reads_seen=%llu bases_seen=%llu reads_masked=%llu bases_masked=%llu bases_already_unknown=%llu\n",
                since_start(), (unsigned long long)bm[0], (unsigned long long)bm[1], (unsigned long long)bm[2], (unsigned long long)bm[3], (unsigned long long)bm[4]);
    }
    if (verbose && poly.min_complexity) { // (of the one pass over the file, like the lines beside it)
        uint64_t cx[4] = {};
        if (drprg_hip_complexity_info(ctx, cx) == 0)
            std::fprintf(stderr, "[drprg-hip +%.3fs] complexity filter: reads_seen=%llu bases_seen=%llu reads_dropped=%llu bases_dropped=%llu\n", since_start(),
                (unsigned long long)cx[0], (unsigned long long)cx[1], (unsigned long long)cx[2], (unsigned long long)cx[3]);
    }
    if (verbose && decoy.any()) {
        uint64_t di[8] = {};
        if (drprg_hip_decoy_info(ctx, di) == 0)
            std::fprintf(stderr, "[drprg-hip +%.3fs] decoy screen: kmers=%llu reads_seen=%llu bases_seen=%llu reads_dropped=%llu bases_dropped=%llu\n", since_start(),
                (unsigned long long)di[0], (unsigned long long)di[2], (unsigned long long)di[3], (unsigned long long)di[4], (unsigned long long)di[5]);
    }
    if (verbose && (min_read_len || max_read_len || min_read_qual_milli)) {
        uint64_t fi[8] = {};
        if (drprg_hip_read_filter_info(ctx, fi) == 0)
            std::fprintf(stderr, "[drprg-hip +%.3fs] read filter: reads_seen=%llu bases_seen=%llu dropped_short=%llu dropped_long=%llu dropped_low_qual=%llu "
                                 "reads_kept=%llu bases_kept=%llu (T=%llu)\n", since_start(), (unsigned long long)fi[0], (unsigned long long)fi[1],
                (unsigned long long)fi[2], (unsigned long long)fi[3], (unsigned long long)fi[4], (unsigned long long)fi[5], (unsigned long long)fi[6],
                (unsigned long long)fi[7]);
    }
    if (pair.any()) { // read-through adapters cut by mate overlap on the resident sample (include/drprg_hip.h "mate overlap"); never a silent unpaired run
        uint64_t out[12] = {};
        if (int rc = drprg_hip_pair_overlap(ctx, out)) die(std::string("--mate: ") + drprg_hip_last_error(ctx), -rc);
        if (verbose) drprg::PairArgs::report(out, [](const char* line) { std::fprintf(stderr, "[drprg-hip +%.3fs] %s\n", since_start(), line); });
        if (pair.merge && verbose) { // (include/drprg_hip.h "mate merging")
            uint64_t mg[8] = {};
            if (int rc = drprg_hip_pair_merge_info(ctx, mg)) die(std::string("--pair-merge: ") + drprg_hip_last_error(ctx), -rc);
            drprg::PairArgs::report_merge(mg, [](const char* line) { std::fprintf(stderr, "[drprg-hip +%.3fs] %s\n", since_start(), line); });
        }
    }
    if (pair.dedup_pairs) { // duplicate pairs dropped from the resident sample (include/drprg_hip.h "duplicate pairs")
        uint64_t out[8] = {};
        if (int rc = drprg_hip_dedup_pairs(ctx, 64, out)) die(std::string("--dedup-pairs: ") + drprg_hip_last_error(ctx), -rc);
        if (verbose) drprg::PairArgs::report_dedup(out, [](const char* line) { std::fprintf(stderr, "[drprg-hip +%.3fs] %s\n", since_start(), line); });
    }
    if (dedup) { // exact duplicates dropped from the resident sample (include/drprg_hip.h "duplicate reads"); never a silent full run
        uint64_t out[4] = { 0, 0, 0, 0 };
        if (int rc = drprg_hip_dedup(ctx, 64, out)) die(std::string("--dedup: ") + drprg_hip_last_error(ctx), -rc);
        if (verbose)
            std::fprintf(stderr, "[drprg-hip +%.3fs] dedup: reads_before=%llu bases_before=%llu reads_kept=%llu bases_kept=%llu\n", since_start(),
                (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3]);
    }
    if (subsample) { // the resident sample cut to the target depth at random (include/drprg_hip.h "random subsample"); never a silent full run
        const uint64_t target = (uint64_t)(subsample_covg * (double)mo.genome_size);
        uint64_t out[4] = { 0, 0, 0, 0 };
        if (int rc = drprg_hip_subsample(ctx, target, seed, out)) die(std::string("--subsample-covg: ") + drprg_hip_last_error(ctx), -rc);
        if (verbose)
            std::fprintf(stderr, "[drprg-hip +%.3fs] subsample: reads_before=%llu bases_before=%llu reads_kept=%llu bases_kept=%llu (target %llu bases, seed %llu)\n",
                since_start(), (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3],
                (unsigned long long)target, (unsigned long long)seed);
    }
    if (qc.any()) { // the report of the one pass over the file, with the counts of --dedup and --subsample-covg: a second pass maps resident reads
        if (int rc = drprg_hip_write_qc_json(ctx, qc.json.c_str(), sample.c_str())) die(std::string("--qc-json: ") + drprg_hip_last_error(ctx), -rc);
        if (verbose) qc.report(ctx, [](const char* line) { std::fprintf(stderr, "[drprg-hip +%.3fs] %s\n", since_start(), line); });
    }
    {
        // discover (/root/reference/src/predict.rs:247-256): candidate regions of every locus' called consensus, then a host-side
        // pile-up of the reads over them (whole strings with -I, column-wise majority of aligned strings without).  Novel variants update the PRG (what MakePrg::update does with
        // make_prg + mafft in the reference, src/predict.rs:260-284, here a new site per variant: -m/-M are not needed), the updated
        // PRG is indexed in the output directory and the reads are mapped again against it.
        std::string ddir = outdir + "/discover";
        mkdir(ddir.c_str(), 0777);
        uint32_t found[3] = { 0, 0, 0 };
        if (int rc = drprg_hip_discover_reads(ctx, input.c_str(), (index + "/genes.fa").c_str(), ddir.c_str(), sample.c_str(), 1, found))
            die(drprg_hip_last_error(ctx), -rc);
        if (verbose || found[1]) {
            uint64_t ri[4] = { 0, 0, 0, 0 };
            drprg_hip_resident_info(ctx, ri);
            std::fprintf(stderr, "[drprg-hip +%.3fs] discover: %u candidate region(s), %u novel variant(s) in %u locus/loci (reads %s)\n", since_start(), found[0],
                found[1], found[2], ri[3] ? "resident in device memory" : "from the file");
        }
        if (found[1]) {
            const std::string updated = outdir + "/updated.dr.prg";
            uint32_t applied = 0;
            if (int rc = drprg_hip_update_prg(ctx, updated.c_str(), &applied)) die(drprg_hip_last_error(ctx), -rc);
            if (applied) {
                if (int rc = drprg_hip_index(updated.c_str(), w, k, threads)) die(drprg_hip_last_error(nullptr), -rc);
                // (the new context opens BEFORE the old one closes: the page-locked ingest blocks of the process go back to the
                // driver with its last context, and pinning them again costs more than the second index does in HBM)
                drprg_hip_ctx* next = devices.size() > 1 ? drprg_hip_open_multi(updated.c_str(), w, k, devices.data(), (int)devices.size(), 1)
                                                         : drprg_hip_open(updated.c_str(), w, k, device);
                if (!next) die(std::string("cannot open the updated PRG: ") + drprg_hip_last_error(nullptr));
                if (int rc = drprg_hip_set_opts(next, &mo)) die(drprg_hip_last_error(next), -rc);
                drprg_hip_set_threads(next, threads);
                drprg_hip_set_input_format(next, packed_input()); // the parser threads pack the reads to 2 bits (DRPRG_HIP_INPUT=ascii: one byte per base)
                if (int rc = drprg_hip_set_read_filter(next, min_read_len, max_read_len, min_read_qual_milli)) die(drprg_hip_last_error(next), -rc);
                if (int rc = drprg_hip_set_read_trim(next, trim_front, trim_tail, trim_qual_milli, trim_window)) die(drprg_hip_last_error(next), -rc);
                if (int rc = drprg_hip_set_base_mask(next, mask_qual)) die(drprg_hip_last_error(next), -rc);
                if (int rc = poly.set_on(next, drprg_hip_set_poly_trim, drprg_hip_set_min_complexity)) die(drprg_hip_last_error(next), -rc);
                if (adapters.any())
                    if (int rc = adapters.set_on(next, drprg_hip_set_adapters, drprg_hip_set_adapters2)) die(drprg_hip_last_error(next), -rc);
                // the reads again, against the updated index: from HBM if the first context kept them all, else from the file
                const int from_hbm = drprg_hip_map_resident(next, ctx);
                if (from_hbm != 0 && from_hbm != -61 /* ENODATA */) die(drprg_hip_last_error(next), -from_hbm);
                if (from_hbm != 0 && pair.any()) die("--mate: the cut reads are no longer resident in device memory for the second pass", 61);
                drprg_hip_close(ctx);
                ctx = next;
                if (from_hbm != 0 && decoy.any()) // (the file again: it is screened again)
                    if (int rc = decoy.set_on(ctx, drprg_hip_set_decoy)) die(drprg_hip_last_error(ctx), -rc);
                if (from_hbm != 0)
                    if (int rc = drprg_hip_map_fastx(ctx, input.c_str())) die(drprg_hip_last_error(ctx), -rc);
                if (verbose)
                    std::fprintf(stderr, "[drprg-hip +%.3fs] %u novel site(s) added to %s; reads mapped again (%s)\n", since_start(), applied, updated.c_str(),
                        from_hbm == 0 ? "resident in device memory" : "from the file");
            }
        }
    }
    const std::string pandora_vcf = outdir + "/pandora_genotyped.vcf";
    if (int rc = drprg_hip_genotype(ctx, (index + "/genes.fa").c_str(), pandora_vcf.c_str(), "sample")) die(drprg_hip_last_error(ctx), -rc);
    if (verbose) {
        uint64_t c[8];
        uint32_t gi[4];
        drprg_hip_counters(ctx, c);
        drprg_hip_genotype_info(ctx, gi);
        std::fprintf(stderr, "[drprg-hip +%.3fs] reads=%llu hits=%llu clusters=%llu exp_depth_covg=%u loci_present=%u records=%u\n",
            since_start(), (unsigned long long)c[0], (unsigned long long)c[3], (unsigned long long)c[4], gi[0], gi[2], gi[3]);
        uint64_t bi[4] = { 0, 0, 0, 0 };
        if (drprg_hip_bam_info(ctx, bi) == 0 && bi[0])
            std::fprintf(stderr, "[drprg-hip +%.3fs] bam: records=%llu skipped=%llu (secondary / supplementary) reverse-complemented=%llu blocks converted on the device=%llu\n",
                since_start(), (unsigned long long)bi[0], (unsigned long long)bi[1], (unsigned long long)bi[2], (unsigned long long)bi[3]);
    }
    drprg_hip_close(ctx);
    if (verbose) std::fprintf(stderr, "[drprg-hip +%.3fs] device context closed\n", since_start());
    char err[1024] = { 0 };
    const std::string out_vcf = outdir + "/" + sample + ".drprg.vcf", out_json = outdir + "/" + sample + ".drprg.json";
    if (int rc = drprg_hip_annotate(index.c_str(), pandora_vcf.c_str(), out_vcf.c_str(), &ao, err, sizeof err)) die(err, -rc);
    if (verbose) std::fprintf(stderr, "[drprg-hip +%.3fs] panel annotated: %s\n", since_start(), out_vcf.c_str());
    // <sample>.drprg.bcf: the file the reference leaves (/root/reference/src/predict.rs:429-431); the text VCF stays beside it
    if (int rc = drprg_hip_vcf_to_bcf(out_vcf.c_str(), (outdir + "/" + sample + ".drprg.bcf").c_str(), err, sizeof err)) die(err, -rc);
    if (int rc = drprg_hip_report_json(index.c_str(), out_vcf.c_str(), out_json.c_str(), sample.c_str(), -1, nullptr, err, sizeof err)) die(err, -rc);
    if (verbose) std::fprintf(stderr, "[drprg-hip +%.3fs] wrote %s\n", since_start(), out_json.c_str());
    // Every output file is closed.  Leave without the static destructors of the HIP runtime: measured (9 runs each, one box)
    // 0.15 s between the line above and the parent seeing the exit with `return 0`, 0.001 s this way for a sample without a
    // novel variant (with one, the kernel still takes ~0.13 s to take the process apart; hipDeviceReset first changes nothing).
    std::fflush(nullptr);
    // Not when anything is evidently attached that does its work from exit handlers (a profiler's output files, a sanitizer's
    // report, a preloaded library): then the process returns normally.  DRPRG_HIP_SLOW_EXIT=1 forces the normal return,
    // DRPRG_HIP_FAST_EXIT=0 as well.
    auto set = [](const char* name) { const char* e = std::getenv(name); return e && *e; };
    auto on = [](const char* name) { const char* e = std::getenv(name); return e && *e && *e != '0'; };
    bool tool = set("LD_PRELOAD") || set("ROCP_TOOL_LIBRARIES") || set("ROCPROFILER_REGISTER_FORCE_LOAD") || set("ROCPROF_OUTPUT_PATH")
        || set("ASAN_OPTIONS") || set("UBSAN_OPTIONS") || set("LSAN_OPTIONS") || set("GCOV_PREFIX") || set("LLVM_PROFILE_FILE");
#if defined(__SANITIZE_ADDRESS__)
    tool = true;
#endif
    if (const char* e = std::getenv("DRPRG_HIP_FAST_EXIT"); e && *e == '0') tool = true;
    if (tool || on("DRPRG_HIP_SLOW_EXIT")) return 0;
    _exit(0);
}
