// Batched threshold matching through include/iris_hip.hpp's TemplateBatchEngine::matches:
//   template_batch_matches <out file> <nq> <n> <seed> <layout> <threshold>
// The database holds n generated templates (seed); query q has pattern limb i =
// (i + 1) * 0x9E3779B97F4A7C15 * (2 q + 1) ^ (q << 7) and mask limb i =
// (i + 3) * 0xD1B54A32D192ED03 * (2 q + 5) | 0x8000000000000001.  The out file receives, per
// query, as u64 / iris_match_t records: count, the whole list; then per query: count, the 2 lowest
// (cap = 2); then the nq counts of a counts-only call (cap = 0).  All with index_base 7.
// tests/test_gpu_template_batch_matches.py compares them with the CPU oracle.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

static bool put(std::FILE *f, const mic::Matches &m) {
    return std::fwrite(&m.count, sizeof m.count, 1, f) == 1 &&
           std::fwrite(m.list.data(), sizeof(mic::Match), m.list.size(), f) == m.list.size();
}

int main(int argc, char **argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s <out file> <nq> <n> <seed> <layout> <threshold>\n", argv[0]);
        return 2;
    }
    const uint32_t nq = (uint32_t)std::atoi(argv[2]);
    const uint64_t n = (uint64_t)std::atoll(argv[3]), seed = (uint64_t)std::atoll(argv[4]);
    const int layout = std::atoi(argv[5]);
    const double threshold = std::atof(argv[6]);
    try {
        mic::Device &dev = mic::Device::default_device();
        mic::Database db(dev, IRIS_KIND_TEMPLATES, n, layout);
        db.generate(n, seed, 0);
        std::vector<mic::Template> queries(nq);
        for (uint32_t q = 0; q < nq; ++q)
            for (std::size_t i = 0; i < queries[q].pattern.limbs.size(); ++i) {
                queries[q].pattern.limbs[i] = ((uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull * (2 * q + 1)) ^ ((uint64_t)q << 7);
                queries[q].mask.limbs[i] = ((uint64_t)(i + 3) * 0xD1B54A32D192ED03ull * (2 * q + 5)) | 0x8000000000000001ull;
            }
        mic::TemplateBatchEngine engine(queries, dev);
        const std::vector<mic::Matches> all = engine.matches(db, threshold, 0, n, 7);
        const std::vector<mic::Matches> low = engine.matches(db, threshold, 0, n, 7, 2);
        const std::vector<mic::Matches> cnt = engine.matches(db, threshold, 0, n, 7, 0);
        if (all.size() != nq || low.size() != nq || cnt.size() != nq) return 3;
        for (uint32_t q = 0; q < nq; ++q)
            if (all[q].list.size() != all[q].count || low[q].count != all[q].count || cnt[q].count != all[q].count ||
                !cnt[q].list.empty())
                return 3;

        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 4;
        bool ok = true;
        for (uint32_t q = 0; q < nq; ++q) ok = ok && put(f, all[q]);
        for (uint32_t q = 0; q < nq; ++q) ok = ok && put(f, low[q]);
        for (uint32_t q = 0; q < nq; ++q) ok = ok && std::fwrite(&cnt[q].count, sizeof cnt[q].count, 1, f) == 1;
        std::fclose(f);
        return ok ? 0 : 4;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
