// Top-k through include/iris_hip.hpp on generated databases:
//   topk <out file> <n> <seed> <layout> <k>
// Templates: a database of n generated templates (seed); the query is generated template 3 of
// seed + 1 with pattern limb 0 inverted.  TemplateEngine::topk runs over records [1, n) with
// index_base 1000.
// Resolver: a database of n generated masks (seed), the query mask is all ones, two share arrays
// share[p][e] = (e * 2654435761 >> 7) + 12345 p (mod 2^16); MasksEngine::topk over all n records
// (index_base 7) must equal resolver_topk over the engine's own rows, and topk_merge of the two
// halves' lists the list of the whole.
// The out file receives, as u64 / iris_match_t records: count, the template list; count, the
// resolver list.  tests/test_gpu_topk.py compares them with the Python mirror's results.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

static bool put(std::FILE *f, const std::vector<mic::Match> &m) {
    const uint64_t count = m.size();
    return std::fwrite(&count, sizeof count, 1, f) == 1 && std::fwrite(m.data(), sizeof(mic::Match), m.size(), f) == m.size();
}

static bool same(const std::vector<mic::Match> &a, const std::vector<mic::Match> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(mic::Match)) == 0);
}

int main(int argc, char **argv) {
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s <out file> <n> <seed> <layout> <k>\n", argv[0]);
        return 2;
    }
    const uint64_t n = (uint64_t)std::atoll(argv[2]), seed = (uint64_t)std::atoll(argv[3]);
    const int layout = std::atoi(argv[4]);
    const uint32_t k = (uint32_t)std::atoi(argv[5]);
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
        const std::vector<mic::Match> tlist = te.topk(tdb, k, 1, n - 1, 1000);
        if (tlist.size() != std::min<uint64_t>(k, n - 1)) return 3;

        mic::Database mdb(dev, IRIS_KIND_MASKS, n, layout);
        mdb.generate(n, seed, 0);
        mic::Bits ones;
        for (auto &l : ones.limbs) l = ~uint64_t(0);
        mic::MasksEngine me(ones, dev);
        std::vector<mic::Rotations> den(n);
        me.batch_process(den, mdb, 0);
        const size_t bytes = n * mic::ROTATIONS * sizeof(uint16_t);
        std::vector<uint16_t> host(n * mic::ROTATIONS);
        void *dptr[3] = {nullptr, nullptr, nullptr};
        for (int p = 0; p < 3; ++p) mic::check(iris_device_alloc(dev.handle(), bytes, &dptr[p]));
        for (int p = 0; p < 2; ++p) {
            for (uint64_t e = 0; e < n * mic::ROTATIONS; ++e)
                host[e] = (uint16_t)((((e * 2654435761ull) & 0xFFFFFFFFull) >> 7) + 12345ull * (uint64_t)p);
            mic::check(iris_memcpy_h2d(dev.handle(), dptr[p], host.data(), bytes));
        }
        mic::check(iris_memcpy_h2d(dev.handle(), dptr[2], den[0].data(), bytes));
        const std::vector<const uint16_t *> shares = {(const uint16_t *)dptr[0], (const uint16_t *)dptr[1]};
        const std::vector<mic::Match> rlist = me.topk(mdb, shares, k, 0, n, 7);
        const std::vector<mic::Match> plain = mic::resolver_topk(dev, shares, (const uint16_t *)dptr[2], n, k, 7);
        // the two halves' lists, merged on the host
        const uint64_t half = n / 2;
        std::vector<mic::Match> parts = mic::resolver_topk(dev, shares, (const uint16_t *)dptr[2], half, k, 7);
        const std::vector<const uint16_t *> upper = {shares[0] + half * mic::ROTATIONS, shares[1] + half * mic::ROTATIONS};
        const std::vector<mic::Match> hi =
            mic::resolver_topk(dev, upper, (const uint16_t *)dptr[2] + half * mic::ROTATIONS, n - half, k, 7 + half);
        parts.insert(parts.end(), hi.begin(), hi.end());
        const std::vector<mic::Match> merged = mic::topk_merge(parts, k);
        for (int p = 0; p < 3; ++p) mic::check(iris_device_free(dev.handle(), dptr[p]));
        if (!same(rlist, plain)) return 4;
        if (!same(rlist, merged)) return 5;

        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 6;
        const bool ok = put(f, tlist) && put(f, rlist);
        if (std::fclose(f) != 0 || !ok) return 7;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
