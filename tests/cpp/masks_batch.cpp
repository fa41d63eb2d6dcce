// A MasksBatchEngine (include/iris_hip.hpp) on a generated masks database:
//   masks_batch <out file> <nq> <n> <seed> <layout>
// Query q is limb i -> (i + 1) * 0x9E3779B97F4A7C15 * (2 q + 1) ^ (q << 7); the database holds
// n + 57 generated masks and the batch runs over records [57, 57 + n).  The nq * n rows of 31 u16
// (query-major) are written to <out file>; tests/test_gpu_masks_batch.py compares them with the
// rows the Python side computes.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "iris_hip.hpp"

namespace mic = mpc_iris_code;

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
        mic::Database db(dev, IRIS_KIND_MASKS, n + 57, layout);
        db.generate(n + 57, seed, 0);
        std::vector<mic::Bits> queries(nq);
        for (uint32_t q = 0; q < nq; ++q)
            for (std::size_t i = 0; i < queries[q].limbs.size(); ++i)
                queries[q].limbs[i] = ((uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull * (2 * q + 1)) ^ ((uint64_t)q << 7);
        mic::MasksBatchEngine engine(queries, dev);
        if (engine.nq() != nq) return 3;
        std::vector<mic::Rotations> out;
        engine.batch_process(out, db, 57, n);
        if (out.size() != (std::size_t)nq * n) return 3;
        std::FILE *f = std::fopen(argv[1], "wb");
        if (!f) return 4;
        const std::size_t wrote = std::fwrite(out.data(), sizeof(mic::Rotations), out.size(), f);
        std::fclose(f);
        return wrote == out.size() ? 0 : 4;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
