// Batched top-k through include/iris_hip.hpp's TemplateBatchEngine::topk:
//   template_batch_topk <out file> <nq> <n> <seed> <layout>
// The database holds n generated templates (seed); query q has pattern limb i =
// (i + 1) * 0x9E3779B97F4A7C15 * (2 q + 1) ^ (q << 7) and mask limb i =
// (i + 3) * 0xD1B54A32D192ED03 * (2 q + 5) | 0x8000000000000001.  The out file receives, for
// k = 2 and then k = 64, per query: the count as u64 and the list's iris_match_t records.  All
// with index_base 7.  tests/test_gpu_template_batch_topk.py compares them with the CPU oracle.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

static bool put(std::FILE *f, const std::vector<mic::Match> &list) {
    const uint64_t count = list.size();
    return std::fwrite(&count, sizeof count, 1, f) == 1 &&
           std::fwrite(list.data(), sizeof(mic::Match), list.size(), f) == list.size();
}

int main(int argc, char **argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s <out file> <nq> <n> <seed> <layout>\n", argv[0]);
        return 2;
    }
    const uint32_t nq = (uint32_t)std::atoi(argv[2]);
    const uint64_t n = (uint64_t)std::atoll(argv[3]), seed = (uint64_t)std::atoll(argv[4]);
    const int layout = std::atoi(argv[5]);
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
        const std::vector<std::vector<mic::Match>> two = engine.topk(db, 2, 0, n, 7);
        const std::vector<std::vector<mic::Match>> full = engine.topk(db, 64, 0, n, 7);
        if (two.size() != nq || full.size() != nq) return 3;
        for (uint32_t q = 0; q < nq; ++q)
            if (two[q].size() > 2 || full[q].size() > 64) return 3;

        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 4;
        bool ok = true;
        for (uint32_t q = 0; q < nq; ++q) ok = ok && put(f, two[q]);
        for (uint32_t q = 0; q < nq; ++q) ok = ok && put(f, full[q]);
        std::fclose(f);
        return ok ? 0 : 4;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
