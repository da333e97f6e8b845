// decoy_args.h -- --decoy FASTA (repeatable), --decoy-k K, --decoy-min-frac F, --decoy-min-kmers M as `pandora map | discover` and
// `drprg predict` take them (include/drprg_hip.h "decoy screen").  Every check that needs no device is made here, so that a usage error is
// one before a device is opened: each function returns the text of the error, which names the flag, or nothing.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace drprg {

struct DecoyArgs {
    std::vector<std::string> files;
    uint32_t k = 0, frac_milli = 0, min_kmers = 0; // (0: the rule's defaults, 31, 0.5 and 1)
    bool k_given = false, frac_given = false, kmers_given = false;
    bool any() const { return !files.empty(); }

    std::string add(const std::string& path)
    {
        if (files.size() >= 8) return "--decoy: at most 8 decoy files, " + path + " is the ninth";
        if (path.empty()) return "--decoy needs a FASTA file";
        files.push_back(path);
        return {};
    }
    static bool number(const std::string& v, uint64_t& n)
    {
        n = 0;
        if (v.empty()) return false;
        for (char c : v) {
            if (c < '0' || c > '9' || n > 1000000000ull) return false;
            n = n * 10 + (uint64_t)(c - '0');
        }
        return true;
    }
    std::string set_k(const std::string& v)
    {
        uint64_t n = 0;
        if (!number(v, n) || n < 9 || n > 31) return "--decoy-k needs a k-mer length of 9 to 31, not " + v;
        k = (uint32_t)n;
        k_given = true;
        return {};
    }
    // a decimal in (0, 1] with at most three places, held as thousandths
    std::string set_frac(const std::string& v)
    {
        const std::string bad = "--decoy-min-frac needs a decimal fraction in (0, 1] with at most 3 places, not " + v;
        size_t i = 0;
        uint64_t whole = 0, frac = 0, places = 0;
        bool digit = false;
        for (; i < v.size() && v[i] >= '0' && v[i] <= '9'; ++i, digit = true)
            if ((whole = whole * 10 + (uint64_t)(v[i] - '0')) > 1000) return bad;
        if (i < v.size() && v[i] == '.')
            for (++i; i < v.size() && v[i] >= '0' && v[i] <= '9'; ++i, ++places, digit = true) {
                if (places >= 3) return bad;
                frac = frac * 10 + (uint64_t)(v[i] - '0');
            }
        if (!digit || i != v.size()) return bad;
        for (; places < 3; ++places) frac *= 10;
        const uint64_t milli = whole * 1000 + frac;
        if (milli < 1 || milli > 1000) return bad;
        frac_milli = (uint32_t)milli;
        frac_given = true;
        return {};
    }
    std::string set_kmers(const std::string& v)
    {
        uint64_t n = 0;
        if (!number(v, n) || n < 1 || n > 0xFFFFFFFFull) return "--decoy-min-kmers needs a number of k-mers of at least 1, not " + v;
        min_kmers = (uint32_t)n;
        kmers_given = true;
        return {};
    }
    // once every flag has been read
    std::string check() const
    {
        if (any()) return {};
        if (k_given) return "--decoy-k belongs to --decoy";
        if (frac_given) return "--decoy-min-frac belongs to --decoy";
        if (kmers_given) return "--decoy-min-kmers belongs to --decoy";
        return {};
    }
    // the settings to a context (the entry is passed in: this header needs no library)
    template <typename Ctx, typename Set> int set_on(Ctx* ctx, Set set_decoy) const
    {
        std::vector<const char*> p;
        for (const std::string& s : files) p.push_back(s.c_str());
        return set_decoy(ctx, p.data(), (uint32_t)p.size(), k, frac_milli, min_kmers);
    }
    std::string tag() const // for what identifies a run
    {
        std::string t = "|Y" + std::to_string(k) + "/" + std::to_string(frac_milli) + "/" + std::to_string(min_kmers);
        for (const std::string& s : files) t += "/" + s;
        return t;
    }
};

} // namespace drprg
