// poly_args.h -- --poly-tail, --poly-min-len and --min-complexity as both executables take them (include/drprg_hip.h "poly tails" and
// "read complexity").
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>

namespace drprg {

struct PolyArgs {
    std::string letters;       // --poly-tail LETTERS: distinct letters of ACGT, as given; empty = not set
    uint32_t min_len = 0;      // --poly-min-len M (2..255); 0 = not given: 10 under --poly-tail
    uint32_t min_complexity = 0; // --min-complexity P (1..100); 0 = not set

    bool tails() const { return !letters.empty(); }
    uint32_t tail_min_len() const { return min_len ? min_len : 10u; }

    // each: what is wrong with `v`, or empty (a usage error: exit 2)
    std::string set_letters(const char* v)
    {
        std::string seen;
        for (const char* c = v; *c; ++c) {
            const char u = (char)(*c & 0xDF);
            if (!(*c & 0x40) || (u != 'A' && u != 'C' && u != 'G' && u != 'T')) return std::string("--poly-tail needs letters of ACGT, not ") + v;
            if (seen.find(u) != std::string::npos) return std::string("--poly-tail names a letter once, not ") + v;
            seen += u;
        }
        if (seen.empty()) return "--poly-tail needs at least one letter of ACGT";
        std::sort(seen.begin(), seen.end()); // (one name per set: the cache key's)
        letters = seen;
        return std::string();
    }
    std::string set_min_len(const char* v)
    {
        char* end = nullptr;
        const unsigned long n = std::strtoul(v, &end, 10);
        if (end == v || *end || *v < '0' || *v > '9' || n < 2 || n > 255) return std::string("--poly-min-len needs a whole number of bases from 2 to 255, not ") + v;
        min_len = (uint32_t)n;
        return std::string();
    }
    std::string set_complexity(const char* v)
    {
        char* end = nullptr;
        const unsigned long n = std::strtoul(v, &end, 10);
        if (end == v || *end || *v < '0' || *v > '9' || n < 1 || n > 100) return std::string("--min-complexity needs a whole percentage from 1 to 100, not ") + v;
        min_complexity = (uint32_t)n;
        return std::string();
    }
    // what only shows once every argument is read
    std::string check() const { return min_len && !tails() ? "--poly-min-len without --poly-tail" : std::string(); }
    // the part of pandora's coverage cache key
    std::string tag() const
    {
        return (tails() ? "|G" + letters + "/" + std::to_string(tail_min_len()) : std::string()) + (min_complexity ? "|X" + std::to_string(min_complexity) : std::string());
    }
    // both settings onto a context; the first refusal's return code, or 0
    template <typename SetPoly, typename SetComplexity, typename Ctx>
    int set_on(Ctx* ctx, SetPoly set_poly, SetComplexity set_complexity) const
    {
        if (int rc = set_poly(ctx, tails() ? letters.c_str() : nullptr, tails() ? tail_min_len() : 0)) return rc;
        return set_complexity(ctx, min_complexity);
    }
};

} // namespace drprg
