// Threshold matching through include/iris_hip.hpp on generated databases:
//   matches <out file> <n> <seed> <layout> <template threshold> <resolver threshold>
// Templates: a database of n generated templates (seed); the query is generated template 3 of
// seed + 1 with pattern limb 0 inverted.  TemplateEngine::matches runs over records [1, n) with
// index_base 1000, once for every match and once with cap = 3.
// Resolver: a database of n generated masks (seed), the query mask is all ones, two share arrays
// share[p][e] = (e * 2654435761 >> 7) + 12345 p (mod 2^16); MasksEngine::matches over all n records
// must equal resolver_matches over the engine's own rows.
// The out file receives, as u64 / iris_match_t records: count, the list; count, the 3 lowest;
// count, the resolver list.  tests/test_gpu_matches.py compares them with the CPU oracle.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

static bool put(std::FILE *f, const mic::Matches &m) {
    return std::fwrite(&m.count, sizeof m.count, 1, f) == 1 &&
           std::fwrite(m.list.data(), sizeof(mic::Match), m.list.size(), f) == m.list.size();
}

int main(int argc, char **argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s <out file> <n> <seed> <layout> <template threshold> <resolver threshold>\n", argv[0]);
        return 2;
    }
    const uint64_t n = (uint64_t)std::atoll(argv[2]), seed = (uint64_t)std::atoll(argv[3]);
    const int layout = std::atoi(argv[4]);
    const double threshold = std::atof(argv[5]), rthreshold = std::atof(argv[6]);
    try {
        mic::Device &dev = mic::Device::default_device();
        mic::Database tdb(dev, IRIS_KIND_TEMPLATES, n, layout);
        tdb.generate(n, seed, 0);
        mic::Database qdb(dev, IRIS_KIND_TEMPLATES, 4, layout);
        qdb.generate(4, seed + 1, 0);
        iris_template_t raw;
        mic::check(iris_db_read(qdb.handle(), 3, 1, &raw));
        raw.pattern[0] = ~raw.pattern[0];
        mic::Template query;
        std::memcpy(query.pattern.limbs.data(), raw.pattern, sizeof raw.pattern);
        std::memcpy(query.mask.limbs.data(), raw.mask, sizeof raw.mask);
        mic::TemplateEngine te(query, dev);
        const mic::Matches all = te.matches(tdb, threshold, 1, n - 1, 1000);
        const mic::Matches low = te.matches(tdb, threshold, 1, n - 1, 1000, 3);
        if (all.list.size() != all.count || low.count != all.count) return 3;

        mic::Database mdb(dev, IRIS_KIND_MASKS, n, layout);
        mdb.generate(n, seed, 0);
        mic::Bits ones;
        for (auto &l : ones.limbs) l = ~uint64_t(0);
        mic::MasksEngine me(ones, dev);
        std::vector<mic::Rotations> den(n);
        me.batch_process(den, mdb, 0);
        const size_t elems = (size_t)n * IRIS_ROTATIONS, bytes = elems * sizeof(uint16_t);
        std::vector<uint16_t> share(elems);
        void *dptr[3] = {nullptr, nullptr, nullptr};
        for (int p = 0; p < 3; ++p) mic::check(iris_device_alloc(dev.handle(), bytes, &dptr[p]));
        for (int p = 0; p < 2; ++p) {
            for (size_t e = 0; e < elems; ++e) share[e] = (uint16_t)(((uint32_t)e * 2654435761u >> 7) + 12345u * (uint32_t)p);
            mic::check(iris_memcpy_h2d(dev.handle(), dptr[p], share.data(), bytes));
        }
        mic::check(iris_memcpy_h2d(dev.handle(), dptr[2], den[0].data(), bytes));
        const std::vector<const uint16_t *> shares = {(const uint16_t *)dptr[0], (const uint16_t *)dptr[1]};
        const mic::Matches fused = me.matches(mdb, shares, rthreshold, 0, n, 7);
        const mic::Matches plain = mic::resolver_matches(dev, shares, (const uint16_t *)dptr[2], n, rthreshold, 7);
        for (int p = 0; p < 3; ++p) mic::check(iris_device_free(dev.handle(), dptr[p]));
        if (fused.count != plain.count || fused.list.size() != plain.list.size() ||
            (fused.count && std::memcmp(fused.list.data(), plain.list.data(), fused.list.size() * sizeof(mic::Match)) != 0))
            return 5;

        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 4;
        const bool ok = put(f, all) && put(f, low) && put(f, fused);
        std::fclose(f);
        return ok ? 0 : 4;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
