// Test driver of the batched think through the C++ facade (include/minizero/actor.h): compiled and run on the GPU by tests/test_gpu_think.py, which compares
// the record it prints with the ctypes worker's.
//   think_check <conf> <moves>      createNetwork + createActor, `moves` times think(true), then getRecord(): RECORD line and a THINK line of the counters
// The configuration carries actor_mcts_think_batch_size; the facade adds mz_manual_step=true itself.
#include "minizero/actor.h"
#include <cstdio>
#include <cstdlib>

using namespace minizero;

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: think_check <conf> <moves>" << std::endl; return 1; }
    const std::string conf = argv[1];
    const int moves = atoi(argv[2]);
    config::mzgpuConfigurationString() = conf;
    std::shared_ptr<network::Network> net = network::createNetwork(config::mzgpuConfValue(conf, "nn_file_name"), 0);
    const int n = std::stoi(config::mzgpuConfValue(conf, "actor_num_simulation"));
    std::shared_ptr<actor::BaseActor> a = actor::createActor(uint64_t(n + 1) * net->getActionSize(), net);
    for (int m = 0; m < moves && !a->isEnvTerminal(); ++m) {
        a->think(true, false);
        if (!a->isSearchDone()) { return 3; }
        if (a->isResign()) { break; }
    }
    std::cout << "RECORD " << a->getRecord() << std::endl;
    uint64_t steps = 0, walks = 0, queries = 0;
    if (mz_worker_think_stats(a->handle(), &steps, &walks, &queries) != MZ_OK) { return 4; }
    std::cout << "THINK " << steps << " " << walks << " " << queries << std::endl;
    return 0;
}
