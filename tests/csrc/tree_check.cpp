// Test driver of the tree read-out through the C++ facade (include/minizero/actor.h): compiled and run on the GPU by tests/test_gpu_tree.py, which compares
// what it prints with the ctypes worker's read-out of the same configuration.
//   tree_check <conf> <moves>      createNetwork + createActor, `moves` times think(true), then of the last search:
//     RECORD   getRecord()
//     TREE     getMCTS()->toString(record)
//     DIST     getMCTS()->getSearchDistributionString()
//     NUMSIM   getMCTS()->getNumSimulation()
//     MAXCOUNT action id of selectChildByMaxCount(root)
//     CHILD    one line per visited root child, from a walk over getRootNode()->getChild(i): position among the visited, i, action id, count, getNumChildren()
//     INFO     the two lines of getSearchNodeInfo()
#include "minizero/actor.h"
#include <cstdio>
#include <cstdlib>

using namespace minizero;

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: tree_check <conf> <moves>" << std::endl; return 1; }
    const std::string conf = argv[1];
    const int moves = atoi(argv[2]);
    config::mzgpuConfigurationString() = conf;
    std::shared_ptr<network::Network> net = network::createNetwork(config::mzgpuConfValue(conf, "nn_file_name"), 0);
    const int n = std::stoi(config::mzgpuConfValue(conf, "actor_num_simulation"));
    std::shared_ptr<actor::BaseActor> base = actor::createActor(uint64_t(n + 1) * net->getActionSize(), net);
    std::shared_ptr<actor::ZeroActor> a = std::dynamic_pointer_cast<actor::ZeroActor>(base);
    if (!a) { return 2; }
    for (int m = 0; m < moves && !a->isEnvTerminal(); ++m) {
        a->think(true, false);
        if (!a->isSearchDone()) { return 3; }
    }
    const std::string record = a->getRecord();
    std::shared_ptr<const actor::MCTS> mcts = a->getMCTS();
    std::cout << "RECORD " << record << std::endl;
    std::cout << "TREE " << mcts->toString(record) << std::endl;
    std::cout << "DIST " << mcts->getSearchDistributionString() << std::endl;
    std::cout << "NUMSIM " << mcts->getNumSimulation() << std::endl;
    const actor::MCTSNode* root = mcts->getRootNode();
    const actor::MCTSNode* best = mcts->selectChildByMaxCount(root);
    if (!best || root->isLeaf()) { return 4; }
    std::cout << "MAXCOUNT " << best->getAction().getActionID() << std::endl;
    int visited = 0;
    for (int i = 0; i < root->getNumChildren(); ++i) {
        const actor::MCTSNode* child = root->getChild(i);
        if (!child) { continue; } // unvisited: not read back
        if (!child->displayInTreeLog()) { return 5; }
        std::cout << "CHILD " << visited++ << " " << i << " " << child->getAction().getActionID() << " " << child->getCount() << " " << child->getNumChildren() << std::endl;
    }
    if (root->getChild(root->getNumChildren()) != nullptr) { return 6; }
    std::istringstream info(a->getSearchNodeInfo());
    for (std::string line; std::getline(info, line);) { std::cout << "INFO " << line << std::endl; }
    // a snapshot is the caller's: the next search does not change it
    const std::string before = mcts->toString(record);
    a->think(false, false);
    if (mcts->toString(record) != before) { return 7; }
    return 0;
}
