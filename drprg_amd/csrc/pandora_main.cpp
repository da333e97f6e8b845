// pandora_main.cpp -- drop-in executable for the `pandora` binary drprg shells out to.
//
// Accepts exactly the argv struct Pandora builds (/root/reference/src/lib.rs:479-642):
//   pandora index    -t T -w W -k K <prg>
//   pandora discover -g G --max-covg M -v -o <dir> -t T -w W -k K -c C [-I] [-K] <prg> <query.tsv>
//   pandora map      --genotype --local --gt-conf 0 -v -o <out> -g G --max-covg M --vcf-refs <genes.fa>
//                    -t T -w W -k K -c C [-I] [-K] <prg> <reads>
// and, this build's own, --subsample-covg D [--seed S] on map and discover (include/drprg_hip.h "random subsample"), --dedup on both
// (include/drprg_hip.h "duplicate reads"),
// --min-read-len L, --max-read-len L and --min-read-qual Q on both (include/drprg_hip.h "read filter"),
// --trim-front N, --trim-tail N, --trim-qual Q and --trim-window W on both (include/drprg_hip.h "read trimming"),
// --adapter SEQ (repeatable), --adapter-error E and --adapter-min-overlap O on both (include/drprg_hip.h "adapter trimming"),
// --decoy FASTA (repeatable), --decoy-k K, --decoy-min-frac F and --decoy-min-kmers M on both (include/drprg_hip.h "decoy screen"),
// and writes the files drprg then looks for: <prg>.k<K>.w<W>.idx + kmer_prgs/ (index),
// <dir>/denovo_paths.txt (discover, /root/reference/src/lib.rs:569-577),
// <out>/pandora_genotyped.vcf (map, /root/reference/src/lib.rs:644-646).
// Diagnostics go to stderr, progress to stdout (drprg redirects stdout to a log file); non-zero exit
// on failure (/root/reference/src/lib.rs:497-506).  Use it with `drprg predict -p <this file>`.
#include "../../include/drprg_hip.h"
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "adapter_args.h"
#include "decoy_args.h"
#include "mask_args.h"
#include "pair_args.h"
#include "qc_args.h"
#include "poly_args.h"

namespace {

// 2-bit packed ingest (include/drprg_hip.h "packed reads") unless DRPRG_HIP_INPUT=ascii: a quarter of the bytes to page-lock, to move over
// PCIe and to keep in HBM; same results
static int packed_input()
{
    const char* e = std::getenv("DRPRG_HIP_INPUT");
    return !(e && std::string(e) == "ascii");
}


struct Args {
    std::string cmd;
    int threads = 1, w = 14, k = 15;
    uint32_t min_cluster_size = 10;
    bool illumina = false, genotype = false, local = false, verbose = false, clean = false, binomial = false;
    double error_rate = -1, gt_conf = 1;
    int max_diff = -1;
    uint64_t genome_size = 5000000;
    uint64_t max_covg = 300;
    bool max_covg_given = false;
    // --subsample-covg D [--seed S]: the resident sample cut to D x genome_size bases at random (include/drprg_hip.h "random subsample")
    bool subsample = false, seed_given = false;
    double subsample_covg = 0;
    uint64_t seed = 1;
    // --dedup: exact duplicate reads dropped from the resident sample (include/drprg_hip.h "duplicate reads")
    bool dedup = false;
    drprg::PairArgs pair; // --mate FILE, --pair-min-overlap O, --pair-error E, --pair-clip-overlap (include/drprg_hip.h "mate overlap")
    // --min-read-len L, --max-read-len L, --min-read-qual Q: the read filter (include/drprg_hip.h "read filter"); 0 = not set
    uint64_t min_read_len = 0, max_read_len = 0;
    uint32_t min_read_qual_milli = 0;
    // --trim-front N, --trim-tail N, --trim-qual Q, --trim-window W: read trimming (include/drprg_hip.h "read trimming"); 0 = not set
    uint64_t trim_front = 0, trim_tail = 0;
    uint32_t trim_qual_milli = 0, trim_window = 0;
    uint32_t mask_qual = 0; // --mask-qual Q: base masking (include/drprg_hip.h "base masking"); 0 = not set
    drprg::AdapterArgs adapters; // --adapter SEQ, --adapter-error E, --adapter-min-overlap O (include/drprg_hip.h "adapter trimming")
    drprg::QcArgs qc; // --qc-json FILE, --qc-no-qual (include/drprg_hip.h "read statistics")
    drprg::PolyArgs poly; // --poly-tail LETTERS, --poly-min-len M, --min-complexity P (include/drprg_hip.h "poly tails", "read complexity")
    drprg::DecoyArgs decoy; // --decoy FASTA, --decoy-k K, --decoy-min-frac F, --decoy-min-kmers M (include/drprg_hip.h "decoy screen")
    std::string outdir = "pandora", vcf_refs;
    std::vector<std::string> positional;
    int device = 0;
};

[[noreturn]] void die(const std::string& msg, int code = 1)
{
    std::fprintf(stderr, "pandora (drprg-hip): error: %s\n", msg.c_str());
    std::exit(code);
}

void usage()
{
    std::fprintf(stderr,
        "pandora-compatible front end of the MI355X drprg hot path\n"
        "  pandora index    [-t N] [-w W] [-k K] <prg>\n"
        "  pandora map      [--genotype] [--local] [--gt-conf X] [-v] [-o DIR] [-g SIZE] [--max-covg N | --subsample-covg D [--seed S]]\n"
        "                   [--dedup] [--min-read-len L] [--max-read-len L] [--min-read-qual Q]\n"
        "                   [--mate FILE [--pair-min-overlap O] [--pair-error E] [--pair-clip-overlap | --pair-merge] [--dedup-pairs]]\n"
        "                   [--trim-front N] [--trim-tail N] [--trim-qual Q [--trim-window W]]\n"
        "                   [--adapter SEQ]... [--adapter-error E] [--adapter-min-overlap O] [--adapter-indels] [--front-adapter SEQ]...\n"
        "                   [--poly-tail LETTERS [--poly-min-len M]] [--min-complexity P] [--qc-json FILE [--qc-no-qual]]\n"
        "                   [--mask-qual Q] [--decoy FASTA]... [--decoy-k K] [--decoy-min-frac F] [--decoy-min-kmers M]\n"
        "                   [--vcf-refs FASTA] [-t N] [-w W] [-k K] [-c N] [-I] [-K] [-e RATE] [--max-diff N] <prg> <reads>\n"
        "  pandora discover [same mapping options] <prg> <query.tsv>\n"
        "  --max-covg N: reads are taken in file order up to and including the first one at which (N + 1) x SIZE bases are reached;\n"
        "                the rest is not mapped (default 300; 4294967295 = no cap)\n"
        "                A prefix is a fair sample only of a file in random order: of a coordinate-sorted BAM it holds the start of the\n"
        "                genome alone, and the loci behind it come out absent.  Use --subsample-covg for such a file.\n"
        "  --subsample-covg D [--seed S]: instead of the prefix cap, map every read, keep them in device memory and cut the sample AT RANDOM\n"
        "                to D x SIZE bases: reads in the order of a 64-bit key made from S (default 1) and the read's number, up to and\n"
        "                including the one that reaches the target; the kept reads are mapped afresh.  The default --max-covg gives way\n"
        "                to it; an explicit --max-covg other than 4294967295 beside it is an error.  Needs the whole sample resident\n"
        "                (DRPRG_HIP_KEEP_READS_GB, default 32): the run fails if it is not.\n"
        "  --dedup: behind the mapping pass (and in front of --subsample-covg) every read that is identical to a read before it in the file --\n"
        "                same length, same bases case-insensitively, non-ACGT bases at the same places; forward strand only -- is dropped on the\n"
        "                device and the kept reads are mapped afresh: the run is that of a file of the kept reads.  Needs the whole sample\n"
        "                resident (DRPRG_HIP_KEEP_READS_GB, default 32): the run fails if it is not.\n"
        "  --min-read-len L, --max-read-len L, --min-read-qual Q: reads shorter than L, longer than L or of a mean quality below Q (a decimal\n"
        "                Phred value; the mean is that of the error probabilities, as nanoq and chopper take it) are dropped on the device\n"
        "                before anything else sees them: the run is that of a file of the kept reads.  --min-read-qual needs qualities:\n"
        "                FASTA, or a BAM record without them, is an error under it.\n"
        "  --trim-front N, --trim-tail N, --trim-qual Q, --trim-window W: every read loses N bases at its start and N at its end and, under\n"
        "                --trim-qual (a decimal Phred value in (0, 93]), what lies outside its first and its last window of W bases (1..32,\n"
        "                default 4) whose MEAN PHRED VALUE is at least Q, then end bases below Q -- on the device, in front of the read filter\n"
        "                and everything else: the run is that of a file of the trimmed reads.  A read trimmed to nothing stays a read of no\n"
        "                bases.  --trim-qual needs qualities: FASTA, or a BAM record without them, is an error under it.\n"
        "  --adapter SEQ (up to 4 times; 1 to 64 letters ACGT), --adapter-error E (0 to 0.5, default 0.1), --adapter-min-overlap O (default 3):\n"
        "                every read is cut at the leftmost start at which an adapter matches with at most floor(c * E) substitutions over\n"
        "                the c = min(adapter, rest of the read) letters compared, c >= O -- on the device, behind --trim-* and in front of\n"
        "                everything else.  Needs no qualities.\n"
        "  --adapter-indels: an occurrence may carry insertions and deletions too (edit distance at most floor(m * E) over the whole adapter).\n"
        "  --front-adapter SEQ (up to 4 times; needs --adapter-indels): 5' adapters, cut off the reads' starts behind the 3' cut.\n"
        "                Still missing: anchored adapters, pair overlap, indels inside an adapter that the read's end cuts short.\n"
        "  --poly-tail LETTERS (letters of ACGT, e.g. G or ACGT), --poly-min-len M (2 to 255, default 10): every read loses its longest suffix of\n"
        "                at least M bases that begins with one of the letters and holds at most min(n / 8, 5) other bases -- the tails two-colour\n"
        "                instruments (NextSeq, NovaSeq) leave when a cluster goes dark, which carry HIGH qualities.  On the device, behind --trim-*\n"
        "                and both --adapter sides, in front of everything else: the run is that of a file of the cut reads.  Needs no qualities.\n"
        "  --min-complexity P (a whole percentage, 1 to 100; fastp's default is 30): a read is dropped when fewer than P %% of its neighbouring\n"
        "                base pairs differ (an unknown base differs from every letter) -- on the device, behind --trim-*, --adapter, --poly-tail,\n"
        "                --mask-qual and --min/max-read-*, in front of --decoy.  This build's own rules, after fastp.  Default: off.\n"
        "  --mask-qual Q (a whole Phred value, 1 to 93): every base whose quality is below Q becomes an unknown base -- on the device, behind\n"
        "                --trim-* and --adapter and in front of everything else: the run is that of a file in which those bases are the letter N.\n"
        "                The read keeps its length, its place in the depth arithmetic and its mean quality; only the k-mers that hold a masked\n"
        "                base stop existing.  Needs qualities: FASTA, or a BAM record without them, is an error under it.  A threshold on what the\n"
        "                basecaller claims: at Nanopore qualities a Q of 10 or more leaves few 15-mers.  Default: off.\n"
        "  %s"
        "  %s"
        "  --decoy FASTA (up to 8 times; plain or .gz), --decoy-k K (9 to 31, default 31), --decoy-min-frac F (in (0, 1], default 0.5),\n"
        "                --decoy-min-kmers M (default 1): a read is dropped as a contaminant when at least M of its k-mers, and at least the\n"
        "                fraction F of its k-mers without a letter other than ACGT, are k-mers of the decoy files in either orientation -- on\n"
        "                the device, behind --trim-*, --adapter and --min/max-read-*: the run is that of a file of the kept reads.  This\n"
        "                build's own rule (k-mer containment, as bbduk ref=); sized for mitochondrion, NTM genomes, phiX, not a human genome.\n"
        "  <reads>: FASTA or FASTQ, plain or gzip; or BAM (secondary and supplementary records are skipped, reverse-strand records are\n"
        "           reverse-complemented, alignments are ignored, qualities are looked at by --min-read-qual, --trim-qual and --mask-qual alone)\n"
        "environment: DRPRG_HIP_DEVICE selects the GPU (default 0); DRPRG_HIP_DEVICES=0,1,.. maps on several GPUs of the node\n",
        drprg::QcArgs::usage(), drprg::PairArgs::usage());
}

Args parse(int argc, char** argv)
{
    Args a;
    if (argc < 2) {
        usage();
        std::exit(2);
    }
    a.cmd = argv[1];
    auto need = [&](int& i) -> const char* {
        if (i + 1 >= argc) die(std::string("option ") + argv[i] + " needs a value", 2);
        return argv[++i];
    };
    for (int i = 2; i < argc; ++i) {
        std::string s = argv[i];
        if (s == "-t" || s == "--threads") a.threads = std::atoi(need(i));
        else if (s == "-w") a.w = std::atoi(need(i));
        else if (s == "-k") a.k = std::atoi(need(i));
        else if (s == "-c" || s == "--min-cluster-size") a.min_cluster_size = (uint32_t)std::strtoul(need(i), nullptr, 10);
        else if (s == "-g" || s == "--genome-size") a.genome_size = std::strtoull(need(i), nullptr, 10);
        else if (s == "--max-covg") {
            a.max_covg = std::strtoull(need(i), nullptr, 10);
            a.max_covg_given = true;
        } else if (s == "--subsample-covg") {
            char* end = nullptr;
            const char* v = need(i);
            a.subsample_covg = std::strtod(v, &end);
            if (end == v || *end || !(a.subsample_covg >= 0)) die(std::string("--subsample-covg needs a depth >= 0, not ") + v, 2);
            a.subsample = true;
        } else if (s == "--seed") {
            a.seed = std::strtoull(need(i), nullptr, 10);
            a.seed_given = true;
        } else if (s == "--min-read-len" || s == "--max-read-len") {
            char* end = nullptr;
            const char* v = need(i);
            const uint64_t n = std::strtoull(v, &end, 10);
            if (end == v || *end || *v == '-') die(s + " needs a number of bases, not " + v, 2);
            (s == "--min-read-len" ? a.min_read_len : a.max_read_len) = n;
        } else if (s == "--min-read-qual") {
            char* end = nullptr;
            const char* v = need(i);
            const double q = std::strtod(v, &end);
            if (end == v || *end || !(q >= 0) || q > 93) die(std::string("--min-read-qual needs a mean quality between 0 and 93, not ") + v, 2);
            a.min_read_qual_milli = (uint32_t)(q * 1000.0 + 0.5);
        }
        else if (s == "--trim-front" || s == "--trim-tail") {
            char* end = nullptr;
            const char* v = need(i);
            const uint64_t n = std::strtoull(v, &end, 10);
            if (end == v || *end || *v == '-') die(s + " needs a number of bases, not " + v, 2);
            (s == "--trim-front" ? a.trim_front : a.trim_tail) = n;
        } else if (s == "--trim-qual") {
            char* end = nullptr;
            const char* v = need(i);
            const double q = std::strtod(v, &end);
            if (end == v || *end || !(q > 0) || q > 93) die(std::string("--trim-qual needs a quality above 0 and at most 93, not ") + v, 2);
            a.trim_qual_milli = (uint32_t)(q * 1000.0 + 0.5);
            if (!a.trim_qual_milli) die(std::string("--trim-qual needs a quality of at least 0.001, not ") + v, 2);
        } else if (s == "--trim-window") {
            char* end = nullptr;
            const char* v = need(i);
            const uint64_t n = std::strtoull(v, &end, 10);
            if (end == v || *end || n < 1 || n > 32) die(std::string("--trim-window needs a window of 1 to 32 bases, not ") + v, 2);
            a.trim_window = (uint32_t)n;
        }
        else if (s == "--mask-qual") {
            const std::string e = drprg::parse_mask_qual(need(i), a.mask_qual);
            if (!e.empty()) die(e, 2);
        }
        else if (s == "--adapter") {
            const std::string e = a.adapters.add(need(i));
            if (!e.empty()) die(e, 2);
        } else if (s == "--front-adapter") {
            const std::string e = a.adapters.add_front(need(i));
            if (!e.empty()) die(e, 2);
        } else if (s == "--adapter-indels") a.adapters.indels = true;
        else if (s == "--adapter-error") {
            const std::string e = a.adapters.set_error(need(i));
            if (!e.empty()) die(e, 2);
        } else if (s == "--adapter-min-overlap") {
            const std::string e = a.adapters.set_overlap(need(i));
            if (!e.empty()) die(e, 2);
        }
        else if (s == "--poly-tail") {
            const std::string e = a.poly.set_letters(need(i));
            if (!e.empty()) die(e, 2);
        } else if (s == "--poly-min-len") {
            const std::string e = a.poly.set_min_len(need(i));
            if (!e.empty()) die(e, 2);
        } else if (s == "--min-complexity") {
            const std::string e = a.poly.set_complexity(need(i));
            if (!e.empty()) die(e, 2);
        }
        else if (s == "--decoy") {
            const std::string e = a.decoy.add(need(i));
            if (!e.empty()) die(e, 2);
        } else if (s == "--decoy-k") {
            const std::string e = a.decoy.set_k(need(i));
            if (!e.empty()) die(e, 2);
        } else if (s == "--decoy-min-frac") {
            const std::string e = a.decoy.set_frac(need(i));
            if (!e.empty()) die(e, 2);
        } else if (s == "--decoy-min-kmers") {
            const std::string e = a.decoy.set_kmers(need(i));
            if (!e.empty()) die(e, 2);
        }
        else if (s == "--qc-json") a.qc.json = need(i);
        else if (s == "--qc-no-qual") a.qc.no_qual = true;
        else if (s == "--dedup") a.dedup = true;
        else if (s == "--mate") a.pair.mate = need(i);
        else if (s == "--pair-clip-overlap") a.pair.clip = true;
        else if (s == "--pair-merge") a.pair.merge = true;
        else if (s == "--dedup-pairs") a.pair.dedup_pairs = true;
        else if (s == "--pair-min-overlap") {
            const std::string e = a.pair.set_overlap(need(i));
            if (!e.empty()) die(e, 2);
        } else if (s == "--pair-error") {
            const std::string e = a.pair.set_error(need(i));
            if (!e.empty()) die(e, 2);
        }
        else if (s == "-o" || s == "--outdir") a.outdir = need(i);
        else if (s == "--vcf-refs") a.vcf_refs = need(i);
        else if (s == "--gt-conf") a.gt_conf = std::atof(need(i));
        else if (s == "-e" || s == "--error-rate") a.error_rate = std::atof(need(i));
        else if (s == "-m" || s == "--max-diff") a.max_diff = std::atoi(need(i));
        else if (s == "-I" || s == "--illumina") a.illumina = true;
        else if (s == "--bin") a.binomial = true;
        else if (s == "-K" || s == "--debugging-files") a.clean = false;
        else if (s == "--genotype") a.genotype = true;
        else if (s == "--local") a.local = true;
        else if (s == "-v") a.verbose = true;
        else if (s == "-h" || s == "--help") {
            usage();
            std::exit(0);
        } else if (!s.empty() && s[0] == '-' && s.size() > 1) die("unknown option " + s, 2);
        else a.positional.push_back(s);
    }
    // (usage errors of the two sampling rules: before anything is opened)
    if (a.seed_given && !a.subsample) die("--seed belongs to --subsample-covg", 2);
    if (a.subsample && a.max_covg_given && a.max_covg != 4294967295ull)
        die("--max-covg and --subsample-covg are alternatives (the prefix cap or the random subsample): give one of them", 2);
    if (a.subsample) a.max_covg = 4294967295ull; // the default cap gives way
    if (const std::string e = a.pair.check(a.max_covg_given ? a.max_covg : ~0ull, a.dedup); !e.empty()) die(e, 2);
    if (a.pair.any()) a.max_covg = 4294967295ull; // (to --mate as well)
    if (a.max_read_len && a.max_read_len < a.min_read_len) die("--max-read-len is below --min-read-len: no read can pass", 2);
    if (a.trim_window && !a.trim_qual_milli) die("--trim-window belongs to --trim-qual", 2);
    if (const std::string e = a.adapters.check(); !e.empty()) die(e, 2);
    if (const std::string e = a.decoy.check(); !e.empty()) die(e, 2);
    if (const std::string e = a.poly.check(); !e.empty()) die(e, 2);
    if (const std::string e = a.qc.check(); !e.empty()) die(e, 2);
    if (const char* d = std::getenv("DRPRG_HIP_DEVICE")) a.device = std::atoi(d);
    return a;
}

void make_dirs(const std::string& path)
{
    std::string cur;
    for (size_t i = 0; i <= path.size(); ++i) {
        if (i == path.size() || path[i] == '/') {
            if (!cur.empty() && mkdir(cur.c_str(), 0777) != 0 && errno != EEXIST) die("cannot create directory " + cur);
        }
        if (i < path.size()) cur += path[i];
    }
}

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

drprg_hip_ctx* open_ctx(const Args& a)
{
    // DRPRG_HIP_DEVICES=0,1,2,3: one context over several GPUs of the node (the reads shard by ingest block)
    std::vector<int> devices;
    if (const char* d = std::getenv("DRPRG_HIP_DEVICES"))
        for (const char* p = d; *p;) {
            char* end = nullptr;
            const long v = std::strtol(p, &end, 10);
            if (end == p) break;
            devices.push_back((int)v);
            p = *end ? end + 1 : end;
        }
    drprg_hip_ctx* ctx = devices.size() > 1 ? drprg_hip_open_multi(a.positional[0].c_str(), a.w, a.k, devices.data(), (int)devices.size(), 1)
                                            : drprg_hip_open(a.positional[0].c_str(), a.w, a.k, devices.size() == 1 ? devices[0] : a.device);
    if (!ctx) die(std::string("cannot open index for ") + a.positional[0] + ": " + drprg_hip_last_error(nullptr));
    drprg_hip_map_opts o {};
    o.illumina = a.illumina;
    o.binomial = a.binomial;
    o.error_rate = a.error_rate;
    o.max_diff = a.max_diff;
    o.min_cluster_size = a.min_cluster_size;
    o.genome_size = a.genome_size;
    if (int rc = drprg_hip_set_opts(ctx, &o)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_set_max_covg(ctx, a.max_covg)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_set_read_filter(ctx, a.min_read_len, a.max_read_len, a.min_read_qual_milli)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_set_read_trim(ctx, a.trim_front, a.trim_tail, a.trim_qual_milli, a.trim_window)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_set_base_mask(ctx, a.mask_qual)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = a.poly.set_on(ctx, drprg_hip_set_poly_trim, drprg_hip_set_min_complexity)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_set_read_stats(ctx, a.qc.mode())) die(drprg_hip_last_error(ctx), -rc);
    if (a.adapters.any()) {
        if (int rc = a.adapters.set_on(ctx, drprg_hip_set_adapters, drprg_hip_set_adapters2)) die(drprg_hip_last_error(ctx), -rc);
    }
    if (a.decoy.any())
        if (int rc = a.decoy.set_on(ctx, drprg_hip_set_decoy)) die(drprg_hip_last_error(ctx), -rc);
    drprg_hip_set_threads(ctx, a.threads);
    drprg_hip_set_input_format(ctx, packed_input()); // the parser threads pack the reads to 2 bits (DRPRG_HIP_INPUT=ascii: one byte per base)
    return ctx;
}

int cmd_index(const Args& a)
{
    if (a.positional.size() != 1) die("index needs exactly one PRG file", 2);
    double t0 = now_s();
    int rc = drprg_hip_index(a.positional[0].c_str(), a.w, a.k, a.threads);
    if (rc) die(drprg_hip_last_error(nullptr), -rc);
    std::printf("[pandora-hip] indexed %s (w=%d k=%d) in %.2fs\n", a.positional[0].c_str(), a.w, a.k, now_s() - t0);
    return 0;
}

void report_counters(drprg_hip_ctx* ctx, double secs)
{
    uint64_t c[8];
    drprg_hip_counters(ctx, c);
    std::printf("[pandora-hip] reads=%llu bases=%llu minimizers=%llu hits=%llu clusters=%llu hits_in_clusters=%llu in %.3fs (%.0f reads/s)\n",
        (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3],
        (unsigned long long)c[4], (unsigned long long)c[5], secs, secs > 0 ? (double)c[0] / secs : 0.0);
}

// identifies (PRG file, reads file, mapping parameters): what a cached coverage vector belongs to
std::string run_tag(const Args& a, const std::string& reads)
{
    auto stamp = [](const std::string& p) {
        struct stat st;
        char* rp = realpath(p.c_str(), nullptr);
        std::string s = rp ? rp : p;
        std::free(rp);
        if (stat(p.c_str(), &st) == 0)
            s += ":" + std::to_string((long long)st.st_size) + ":" + std::to_string((long long)st.st_mtim.tv_sec) + "."
                + std::to_string((long long)st.st_mtim.tv_nsec);
        return s;
    };
    return stamp(a.positional[0]) + "|" + stamp(reads) + "|w" + std::to_string(a.w) + "|k" + std::to_string(a.k) + "|c"
        + std::to_string(a.min_cluster_size) + "|I" + std::to_string((int)a.illumina) + "|e" + std::to_string(a.error_rate) + "|m"
        + std::to_string(a.max_diff) + "|g" + std::to_string((unsigned long long)a.genome_size) + "|M" + std::to_string((unsigned long long)a.max_covg)
        + (a.subsample ? "|S" + std::to_string(a.subsample_covg) + "/" + std::to_string((unsigned long long)a.seed) : std::string())
        + (a.dedup ? std::string("|D") : std::string())
        + (a.pair.any() ? "|" + stamp(a.pair.mate) + "|M" + std::to_string(a.pair.min_overlap) + "/" + std::to_string(a.pair.error_milli) + "/"
                  + std::to_string((int)a.pair.clip) + (a.pair.merge ? "/G" : "") + (a.pair.dedup_pairs ? "/P" : "")
                        : std::string())
        + (a.min_read_len || a.max_read_len || a.min_read_qual_milli ? "|F" + std::to_string((unsigned long long)a.min_read_len) + "/"
                  + std::to_string((unsigned long long)a.max_read_len) + "/" + std::to_string(a.min_read_qual_milli)
                                                                     : std::string())
        + (a.trim_front || a.trim_tail || a.trim_qual_milli ? "|T" + std::to_string((unsigned long long)a.trim_front) + "/"
                  + std::to_string((unsigned long long)a.trim_tail) + "/" + std::to_string(a.trim_qual_milli) + "/"
                  + std::to_string(a.trim_qual_milli ? (a.trim_window ? a.trim_window : 4u) : 0u)
                                                            : std::string())
        + (a.adapters.any() ? a.adapters.tag() : std::string()) + a.poly.tag() + (a.mask_qual ? "|B" + std::to_string(a.mask_qual) : std::string())
        + (a.decoy.any() ? a.decoy.tag() : std::string());
}

// The reads stay in HBM after the mapping pass: up to DRPRG_HIP_KEEP_READS_GB per device, default 32, 0 = off.  --subsample-covg and --dedup work on
// the resident sample, so there "off" is an error, not a slower route.
void keep_reads(drprg_hip_ctx* ctx, const Args& a)
{
    double keep_gb = 32;
    if (const char* e = std::getenv("DRPRG_HIP_KEEP_READS_GB")) keep_gb = std::atof(e);
    if (a.subsample || a.dedup || a.pair.any()) drprg_hip_set_ordered_ingest(ctx, 1); // (all three number the reads in file order)
    if (keep_gb > 0) {
        if (int rc = drprg_hip_keep_reads(ctx, (uint64_t)(keep_gb * 1e9))) die(drprg_hip_last_error(ctx), -rc);
    } else if (a.pair.any())
        die("--mate needs the reads resident in device memory: DRPRG_HIP_KEEP_READS_GB=0 switches that off");
    else if (a.subsample)
        die("--subsample-covg needs the reads resident in device memory: DRPRG_HIP_KEEP_READS_GB=0 switches that off");
    else if (a.dedup)
        die("--dedup needs the reads resident in device memory: DRPRG_HIP_KEEP_READS_GB=0 switches that off");
}

// The mapping pass: the reads, and with --mate the second mates behind them and the overlap stage on the resident pairs, in front of
// --dedup.  Fails loudly rather than run unpaired.
void map_reads(drprg_hip_ctx* ctx, const Args& a, const std::string& reads)
{
    if (int rc = a.pair.set_on(ctx)) die(drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_map_fastx(ctx, reads.c_str())) die(drprg_hip_last_error(ctx), -rc);
    if (!a.pair.any()) return;
    if (int rc = drprg_hip_begin_mates(ctx)) die(std::string("--mate: ") + drprg_hip_last_error(ctx), -rc);
    if (int rc = drprg_hip_map_fastx(ctx, a.pair.mate.c_str())) die(drprg_hip_last_error(ctx), -rc);
    uint64_t out[12] = {};
    if (int rc = drprg_hip_pair_overlap(ctx, out)) die(std::string("--mate: ") + drprg_hip_last_error(ctx), -rc);
    if (a.verbose) drprg::PairArgs::report(out, [](const char* line) { std::printf("[pandora-hip] %s\n", line); });
    if (a.pair.merge && a.verbose) {
        uint64_t mg[8] = {};
        if (int rc = drprg_hip_pair_merge_info(ctx, mg)) die(std::string("--pair-merge: ") + drprg_hip_last_error(ctx), -rc);
        drprg::PairArgs::report_merge(mg, [](const char* line) { std::printf("[pandora-hip] %s\n", line); });
    }
    if (!a.pair.dedup_pairs) return;
    uint64_t dd[8] = {};
    if (int rc = drprg_hip_dedup_pairs(ctx, 64, dd)) die(std::string("--dedup-pairs: ") + drprg_hip_last_error(ctx), -rc);
    if (a.verbose) drprg::PairArgs::report_dedup(dd, [](const char* line) { std::printf("[pandora-hip] %s\n", line); });
}

// --dedup: behind the mapping pass, in front of --subsample-covg.  Fails loudly when the sample is not resident.
void dedup(drprg_hip_ctx* ctx, const Args& a)
{
    if (!a.dedup) return;
    uint64_t out[4] = { 0, 0, 0, 0 };
    if (int rc = drprg_hip_dedup(ctx, 64, out)) die(std::string("--dedup: ") + drprg_hip_last_error(ctx), -rc);
    if (a.verbose)
        std::printf("[pandora-hip] dedup: reads_before=%llu bases_before=%llu reads_kept=%llu bases_kept=%llu\n", (unsigned long long)out[0],
            (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3]);
}

// --subsample-covg: behind the mapping pass, before anything reads coverage.  Fails loudly when the sample is not resident.
void subsample(drprg_hip_ctx* ctx, const Args& a)
{
    if (!a.subsample) return;
    const uint64_t target = (uint64_t)(a.subsample_covg * (double)a.genome_size);
    uint64_t out[4] = { 0, 0, 0, 0 };
    if (int rc = drprg_hip_subsample(ctx, target, a.seed, out)) die(std::string("--subsample-covg: ") + drprg_hip_last_error(ctx), -rc);
    if (a.verbose)
        std::printf("[pandora-hip] subsample: reads_before=%llu bases_before=%llu reads_kept=%llu bases_kept=%llu (target %llu bases, seed %llu)\n",
            (unsigned long long)out[0], (unsigned long long)out[1], (unsigned long long)out[2], (unsigned long long)out[3], (unsigned long long)target,
            (unsigned long long)a.seed);
}

// -v: says where the depth cap stopped the pass, if it did
void report_cap(drprg_hip_ctx* ctx, const Args& a)
{
    uint64_t ci[4] = { 0, 0, 0, 0 };
    if (!a.verbose || drprg_hip_max_covg_info(ctx, ci) != 0 || !ci[0]) return;
    std::printf("[pandora-hip] stopped reading at %llu reads: max coverage reached (--max-covg %llu x -g %llu: %llu bases mapped)\n", (unsigned long long)ci[1],
        (unsigned long long)a.max_covg, (unsigned long long)a.genome_size, (unsigned long long)ci[2]);
}

// -v: what a BAM file held
void report_bam(drprg_hip_ctx* ctx, const Args& a)
{
    uint64_t bi[4] = { 0, 0, 0, 0 };
    if (!a.verbose || drprg_hip_bam_info(ctx, bi) != 0 || !bi[0]) return;
    std::printf("[pandora-hip] bam: records=%llu skipped=%llu (secondary / supplementary) reverse-complemented=%llu blocks converted on the device=%llu\n",
        (unsigned long long)bi[0], (unsigned long long)bi[1], (unsigned long long)bi[2], (unsigned long long)bi[3]);
}

// -v: what the read trimming cut, and what the read filter dropped
void report_filter(drprg_hip_ctx* ctx, const Args& a)
{
    uint64_t fi[8] = {};
    if (a.verbose && (a.trim_front || a.trim_tail || a.trim_qual_milli) && drprg_hip_read_trim_info(ctx, fi) == 0)
        std::printf("[pandora-hip] read trimming: reads_seen=%llu bases_seen=%llu reads_lost_base=%llu cut_front=%llu cut_tail=%llu qual_cut_front=%llu "
                    "qual_cut_tail=%llu reads_emptied=%llu\n", (unsigned long long)fi[0], (unsigned long long)fi[1], (unsigned long long)fi[2],
            (unsigned long long)fi[3], (unsigned long long)fi[4], (unsigned long long)fi[5], (unsigned long long)fi[6], (unsigned long long)fi[7]);
    if (a.verbose && !a.adapters.seqs.empty() && drprg_hip_adapter_trim_info(ctx, fi) == 0)
        std::printf("[pandora-hip] adapter trimming: reads_seen=%llu bases_seen=%llu reads_cut=%llu bases_cut=%llu reads_emptied=%llu\n", (unsigned long long)fi[0],
            (unsigned long long)fi[1], (unsigned long long)fi[2], (unsigned long long)fi[3], (unsigned long long)fi[4]);
    if (a.verbose && !a.adapters.front.empty() && drprg_hip_front_adapter_info(ctx, fi) == 0)
        std::printf("[pandora-hip] front adapter trimming: reads_seen=%llu bases_seen=%llu reads_cut=%llu bases_cut=%llu reads_emptied=%llu\n", (unsigned long long)fi[0],
            (unsigned long long)fi[1], (unsigned long long)fi[2], (unsigned long long)fi[3], (unsigned long long)fi[4]);
    if (a.verbose && a.poly.tails() && drprg_hip_poly_trim_info(ctx, fi) == 0)
        std::printf("[pandora-hip] poly tail trimming: reads_seen=%llu bases_seen=%llu reads_cut=%llu bases_cut=%llu reads_emptied=%llu\n", (unsigned long long)fi[0],
            (unsigned long long)fi[1], (unsigned long long)fi[2], (unsigned long long)fi[3], (unsigned long long)fi[4]);
    if (a.verbose && a.mask_qual && drprg_hip_base_mask_info(ctx, fi) == 0)
        std::printf("[pandora-hip] base masking: reads_seen=%llu bases_seen=%llu reads_masked=%llu bases_masked=%llu bases_already_unknown=%llu\n",
            (unsigned long long)fi[0], (unsigned long long)fi[1], (unsigned long long)fi[2], (unsigned long long)fi[3], (unsigned long long)fi[4]);
    if (a.verbose && a.poly.min_complexity && drprg_hip_complexity_info(ctx, fi) == 0)
        std::printf("[pandora-hip] complexity filter: reads_seen=%llu bases_seen=%llu reads_dropped=%llu bases_dropped=%llu\n", (unsigned long long)fi[0],
            (unsigned long long)fi[1], (unsigned long long)fi[2], (unsigned long long)fi[3]);
    if (a.verbose && a.decoy.any() && drprg_hip_decoy_info(ctx, fi) == 0)
        std::printf("[pandora-hip] decoy screen: kmers=%llu reads_seen=%llu bases_seen=%llu reads_dropped=%llu bases_dropped=%llu\n", (unsigned long long)fi[0],
            (unsigned long long)fi[2], (unsigned long long)fi[3], (unsigned long long)fi[4], (unsigned long long)fi[5]);
    if (!a.verbose || !(a.min_read_len || a.max_read_len || a.min_read_qual_milli) || drprg_hip_read_filter_info(ctx, fi) != 0) return;
    std::printf("[pandora-hip] read filter: reads_seen=%llu bases_seen=%llu dropped_short=%llu dropped_long=%llu dropped_low_qual=%llu reads_kept=%llu "
                "bases_kept=%llu (T=%llu)\n", (unsigned long long)fi[0], (unsigned long long)fi[1], (unsigned long long)fi[2], (unsigned long long)fi[3],
        (unsigned long long)fi[4], (unsigned long long)fi[5], (unsigned long long)fi[6], (unsigned long long)fi[7]);
}

// --qc-json: the report of the mapping pass (behind --dedup and --subsample-covg, whose counts it carries), and -v's two lines
void report_qc(drprg_hip_ctx* ctx, const Args& a, const std::string& sample)
{
    if (!a.qc.any()) return;
    if (int rc = drprg_hip_write_qc_json(ctx, a.qc.json.c_str(), sample.c_str())) die(std::string("--qc-json: ") + drprg_hip_last_error(ctx), -rc);
    if (a.verbose) a.qc.report(ctx, [](const char* line) { std::printf("[pandora-hip] %s\n", line); });
}

const char* COVERAGE_CACHE = ".drprg_hip_coverage";

int cmd_map(const Args& a)
{
    if (a.positional.size() != 2) die("map needs <prg> <reads>", 2);
    make_dirs(a.outdir);
    drprg_hip_ctx* ctx = open_ctx(a);
    double t0 = now_s();
    // drprg runs `discover -o <out>/discover` on the same reads and PRG first (/root/reference/src/predict.rs:248-255): if that
    // pass left its coverage vector there, take it instead of streaming the reads again
    const std::string cache = a.outdir + "/discover/" + COVERAGE_CACHE;
    uint64_t cached[8];
    // (--qc-json describes a pass over the reads: with it the pass is made, whatever discover left)
    if (!a.qc.any() && drprg_hip_load_coverage(ctx, cache.c_str(), run_tag(a, a.positional[1]).c_str(), cached) == 0) {
        std::printf("[pandora-hip] coverage of this PRG and these reads taken from %s (reads=%llu bases=%llu hits=%llu): no second mapping pass\n",
            cache.c_str(), (unsigned long long)cached[0], (unsigned long long)cached[1], (unsigned long long)cached[3]);
    } else {
        if (a.subsample || a.dedup || a.pair.any()) keep_reads(ctx, a);
        map_reads(ctx, a, a.positional[1]);
        dedup(ctx, a);
        subsample(ctx, a);
        report_counters(ctx, now_s() - t0);
        report_cap(ctx, a);
        report_bam(ctx, a);
        report_filter(ctx, a);
        report_qc(ctx, a, "sample");
    }
    const std::string vcf = a.outdir + "/pandora_genotyped.vcf";
    if (int rc = drprg_hip_genotype(ctx, a.vcf_refs.empty() ? nullptr : a.vcf_refs.c_str(), vcf.c_str(), "sample"))
        die(drprg_hip_last_error(ctx), -rc);
    uint32_t gi[4];
    drprg_hip_genotype_info(ctx, gi);
    std::printf("[pandora-hip] exp_depth_covg=%u min_kmer_covg=%u loci_present=%u records=%u -> %s\n", gi[0], gi[1], gi[2], gi[3],
        vcf.c_str());
    drprg_hip_close(ctx);
    return 0;
}

int cmd_discover(const Args& a)
{
    if (a.positional.size() != 2) die("discover needs <prg> <query.tsv>", 2);
    make_dirs(a.outdir);
    // query.tsv: one line "sample<TAB>/abs/reads" (/root/reference/src/predict.rs:227-231)
    std::ifstream q(a.positional[1]);
    if (!q) die("cannot open " + a.positional[1]);
    std::string sample, reads;
    if (!(q >> sample >> reads)) die("malformed query file " + a.positional[1]);
    drprg_hip_ctx* ctx = open_ctx(a);
    // pandora discover walks the reads twice (mapping, then the candidate regions); here the second walk is over the blocks the
    // first one left in HBM (up to DRPRG_HIP_KEEP_READS_GB per device, default 32, 0 = read the file again)
    keep_reads(ctx, a);
    double t0 = now_s();
    map_reads(ctx, a, reads);
    dedup(ctx, a);
    subsample(ctx, a);
    report_counters(ctx, now_s() - t0);
    report_cap(ctx, a);
    report_bam(ctx, a);
    report_filter(ctx, a);
    report_qc(ctx, a, sample);
    // The mapping half of discover is the same kernels as `map`; its products are (1) the candidate regions -- stretches of each
    // locus' called consensus that the reads do not support --, (2) the novel variants a host-side pile-up of
    // the reads finds in them, and (3) the coverage vector, kept for the `map` call drprg issues next on the unchanged PRG.
    // denovo_paths.txt lists the loci with novel variants (the caller then runs `make_prg update` on this file,
    // /root/reference/src/lib.rs:279-456): the layout of the example in the reference tree (/root/reference/src/lib.rs:3010-3038),
    // read back in the tests by a line-for-line port of the reference's own parser (/root/reference/src/lib.rs:648-697) for files
    // with several loci, several variants per locus and paths through nested sites.  DRPRG_HIP_DENOVO_PATHS=0: report 0 loci
    // (drprg then keeps the index PRG, /root/reference/src/lib.rs:299-301); the findings are in denovo_variants.tsv either way.
    const char* paths_env = std::getenv("DRPRG_HIP_DENOVO_PATHS");
    const int list_loci = !(paths_env && std::atoi(paths_env) == 0);
    uint32_t found[3] = { 0, 0, 0 };
    if (int rc = drprg_hip_discover_reads(ctx, reads.c_str(), nullptr, a.outdir.c_str(), sample.c_str(), list_loci, found))
        die(drprg_hip_last_error(ctx), -rc);
    if (drprg_hip_save_coverage(ctx, (a.outdir + "/" + COVERAGE_CACHE).c_str(), run_tag(a, reads).c_str()) != 0)
        std::fprintf(stderr, "pandora (drprg-hip): warning: could not keep the coverage vector for `map`: %s\n", drprg_hip_last_error(ctx));
    if (found[1] && !list_loci)
        std::fprintf(stderr,
            "pandora (drprg-hip): WARNING: %u novel variant(s) in %u locus/loci found (%s/denovo_variants.tsv) but denovo_paths.txt reports 0 "
            "loci (DRPRG_HIP_DENOVO_PATHS=0), so the PRG will not be updated.\n", found[1], found[2], a.outdir.c_str());
    uint64_t ri[4] = { 0, 0, 0, 0 };
    drprg_hip_resident_info(ctx, ri);
    std::printf("[pandora-hip] discover: %u candidate regions, %u novel variants in %u loci%s; reads of the second pass %s\n", found[0], found[1], found[2],
        list_loci ? "" : " (not listed in denovo_paths.txt)", ri[3] ? "resident in device memory" : "from the file");
    drprg_hip_close(ctx);
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    Args a = parse(argc, argv);
    if (a.cmd == "index") return cmd_index(a);
    if (a.cmd == "map") return cmd_map(a);
    if (a.cmd == "discover") return cmd_discover(a);
    if (a.cmd == "-h" || a.cmd == "--help") {
        usage();
        return 0;
    }
    usage();
    return 2;
}
