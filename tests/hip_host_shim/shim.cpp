// The one definition of the host shim's globals and of its launch: every workgroup of the grid in turn, one std::thread per lane
// (hip/hip_runtime.h).  Linked into each stand-alone emulation program next to its *_main.cpp.
#include <hip/hip_runtime.h>

#include <thread>
#include <vector>

thread_local dim3 threadIdx, blockIdx;
dim3 blockDim, gridDim;
ShimWorkgroup shim;

void shim_launch(dim3 grid, dim3 block, std::function<void()> fn) {
    gridDim = grid;
    blockDim = block;
    for (unsigned z = 0; z < grid.z; ++z)
        for (unsigned y = 0; y < grid.y; ++y)
            for (unsigned x = 0; x < grid.x; ++x) {
                pthread_barrier_init(&shim.all, nullptr, block.x);
                for (unsigned w = 0; w < (block.x + 63) / 64; ++w) pthread_barrier_init(&shim.wave[w], nullptr, std::min(64u, block.x - 64 * w));
                std::vector<std::thread> lanes;
                for (unsigned t = 0; t < block.x; ++t)
                    lanes.emplace_back([=] {
                        threadIdx = dim3(t, 0, 0);
                        blockIdx = dim3(x, y, z);
                        fn();
                    });
                for (auto& l : lanes) l.join();
                pthread_barrier_destroy(&shim.all);
                for (unsigned w = 0; w < (block.x + 63) / 64; ++w) pthread_barrier_destroy(&shim.wave[w]);
            }
}
