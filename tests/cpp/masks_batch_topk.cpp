// Batched top-k through include/iris_hip.hpp's MasksBatchEngine::topk:
//   masks_batch_topk <out file> <nq> <n> <seed> <layout> <k>
// The database holds n generated masks (seed); query q is masks_batch.cpp's: limb i ->
// (i + 1) * 0x9E3779B97F4A7C15 * (2 q + 1) ^ (q << 7).  Two participants' query-major share arrays
// of nq * n * 31 u16: share[p][e] = (e * 2654435761 >> 7) + 12345 p (mod 2^16).  The out file
// receives, per query, as u64 / iris_match_t records: count, the k-list (index_base 7); then per
// query: count, the list of k = 2.  tests/test_gpu_masks_batch_topk.py compares them with the
// Python mirror's call on the same inputs.
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
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s <out file> <nq> <n> <seed> <layout> <k>\n", argv[0]);
        return 2;
    }
    const uint32_t nq = (uint32_t)std::atoi(argv[2]);
    const uint64_t n = (uint64_t)std::atoll(argv[3]), seed = (uint64_t)std::atoll(argv[4]);
    const int layout = std::atoi(argv[5]);
    const uint32_t k = (uint32_t)std::atoi(argv[6]);
    try {
        mic::Device &dev = mic::Device::default_device();
        mic::Database db(dev, IRIS_KIND_MASKS, n, layout);
        db.generate(n, seed, 0);
        std::vector<mic::Bits> queries(nq);
        for (uint32_t q = 0; q < nq; ++q)
            for (std::size_t i = 0; i < queries[q].limbs.size(); ++i)
                queries[q].limbs[i] = ((uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull * (2 * q + 1)) ^ ((uint64_t)q << 7);
        mic::MasksBatchEngine engine(queries, dev);
        const size_t elems = (size_t)nq * n * IRIS_ROTATIONS, bytes = elems * sizeof(uint16_t);
        std::vector<uint16_t> share(elems);
        void *dptr[2] = {nullptr, nullptr};
        for (int p = 0; p < 2; ++p) {
            mic::check(iris_device_alloc(dev.handle(), bytes, &dptr[p]));
            for (size_t e = 0; e < elems; ++e) share[e] = (uint16_t)(((uint32_t)e * 2654435761u >> 7) + 12345u * (uint32_t)p);
            mic::check(iris_memcpy_h2d(dev.handle(), dptr[p], share.data(), bytes));
        }
        const std::vector<const uint16_t *> shares = {(const uint16_t *)dptr[0], (const uint16_t *)dptr[1]};
        const std::vector<std::vector<mic::Match>> all = engine.topk(db, shares, k, 0, n, 7);
        const std::vector<std::vector<mic::Match>> two = engine.topk(db, shares, 2, 0, n, 7);
        for (int p = 0; p < 2; ++p) mic::check(iris_device_free(dev.handle(), dptr[p]));
        if (all.size() != nq || two.size() != nq) return 3;

        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 4;
        bool ok = true;
        for (uint32_t q = 0; q < nq; ++q) ok = ok && put(f, all[q]);
        for (uint32_t q = 0; q < nq; ++q) ok = ok && put(f, two[q]);
        std::fclose(f);
        return ok ? 0 : 4;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
