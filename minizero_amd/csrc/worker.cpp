// The self-play worker of libmzgpu: the `-mode sp` loop of the reference (ref actor/actor_group.cpp:136-252)
// re-designed around one device-resident search pool per GPU.
//
// Per lock-step cycle (one simulation of every game, ref actor_group.cpp:139-147 / SURVEY.md §3.1):
//   device : expand+backup kernel  ->  PUCT select kernel  ->  network forward (f32 MFMA)
//   host   : per-game candidate lists (legal filter, inverse rotation, the reference's std::sort), leaf
//            environments (copy of the root position + path replay) and feature planes — embarrassingly
//            parallel over games on a thread pool — plus the strictly serial, RNG-ordered per-move logic
//            (root noise, move decision, resign coin, record strings) on one thread.
// The order in which the single mt19937 stream is consumed is the reference's: for actor 0..B-1:
// [root noise] [move decision] [reset: resign coin] [rotation draw].
#include "config.h"
#include "env.h"
#include "net.h"
#include "ext_eval.h"
#include "pool.h"
#include "go_dev.h"
#include "think.h"
#include "tree_read.h"
#include "gumbel.h"
#include "host_threads.h"
#include <pthread.h>
#include <sched.h>
#include <unistd.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <functional>
#include <limits>
#include <mutex>
#include <numeric>
#include <random>
#include <sstream>
#include <thread>
#include <unordered_map>

namespace mz {

namespace {

struct Cand { int action; float policy, logit; };

using ActionInfo = std::vector<std::pair<std::string, std::string>>;

struct Game {
    std::unique_ptr<GameEnv> env, leaf;
    bool enable_resign = true;
    int rot = 0;
    // leaf cache (AlphaZero): filled when the features are built, consumed when the network output arrives
    bool leaf_terminal = false;
    float leaf_eval = 0, leaf_reward = 0;
    int leaf_turn = 1, path_len = 1;
    std::vector<uint8_t> legal;
    // Gumbel root state (ref gumbel_zero.h:18-21); candidates are indices into the root's children
    std::vector<int> candidates;
    int sample_size = 0, simulation_budget = 0;
    int selected = -1; // index of the chosen root child
    uint64_t raw_seen = ~0ull; // rawSerial() of the observation block last sent to the device
    std::vector<ActionInfo> action_info_history;
    // match play (mz_worker_create_match): serial number of a counted game (-1: a filler), the step it started at, the side of its first player, and what
    // the last move did to it — written by handleSearchDone, consumed in slot order by matchAfterMoves
    int m_serial = -1, m_first_side = 0;
    uint64_t m_t0 = 0;
    bool m_acted = false, m_ended = false, m_resigned = false;
    float m_score = 0.0f;
};

// optional host-side phase trace (MZ_TRACE=1): prints per-sub-step averages to stderr when the worker is destroyed
struct PhaseTrace {
    bool on = getenv("MZ_TRACE") != nullptr;
    double acc[20] = {0}, lo[20] = {0}, hi[20] = {0};
    uint64_t cnt[20] = {0};
    const char* names[20] = {"p1.sync", "p1.cand", "p1.expand_launch", "p1.rootread", "p1.serial", "p1.noise_reset", "p1.select_launch", "p2.sync", "p2.leaf",
                             "p2.fwd_launch", "p1.observations", "p1.noise_up", "p1.reset", "p1.upload_roots", "root.flush", "sim.prep", "iter.root", "iter.presim", "iter.simwait", ""};
    void add(int i, double ms)
    {
        if (!cnt[i] || ms < lo[i]) { lo[i] = ms; }
        if (!cnt[i] || ms > hi[i]) { hi[i] = ms; }
        acc[i] += ms; ++cnt[i];
        if (on && i < 18 && ms > 1.5) { fprintf(stderr, "[mz trace] slow %s #%llu: %.3f ms\n", names[i], (unsigned long long)cnt[i], ms); }
    }
    ~PhaseTrace()
    {
        if (!on) { return; }
        for (int i = 0; i < 20; ++i) { if (cnt[i]) { fprintf(stderr, "[mz trace] %-18s calls %8llu  avg %8.4f ms  (min %8.4f, max %8.4f)  total %10.2f ms\n", names[i], (unsigned long long)cnt[i], acc[i] / cnt[i], lo[i], hi[i], acc[i]); } }
    }
};

inline double nowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

std::string escapeSGF(const std::string& s) // ref base_env.h:303-313
{
    std::string out;
    for (char c : s) {
        if (c == '(' || c == ')' || c == '[' || c == ']' || c == '\\') { out += '\\'; }
        out += c;
    }
    return out;
}

} // namespace

// Workers of THIS process per physical device (one-process-for-all-GPUs with MZ_DEVICE_MAP=0,0, tools/multi_worker.py, a facade user with several actor groups): kernels
// that assume a whole idle GPU — the pairs of workgroups per leaf of sim_pre_pair_kernel_mz, which spin on each other — are only used by a worker that is alone on
// its device.  (Another PROCESS on the device cannot be seen from here: there the bounded wait + pairTrouble() of adaptRounds is the net, or mz_sim_round_pairs=false.)
static std::atomic<int> g_workers_on_device[64];

class Worker {
public:
    ~Worker()
    {
        obs_.reset(); // the compressor's threads write into queued lines: they end before anything else goes
        if (counted_device_ >= 0) { g_workers_on_device[counted_device_].fetch_sub(1); }
    }
    int counted_device_ = -1;
    // shared != nullptr: the worker runs on the caller's network (BaseActor::setNetwork's shared_ptr, ref zero_actor.cpp:100-112) instead of its own copy
    // ext != nullptr: no network at all — the caller's code evaluates the leaves (mz_worker_create_external, ext_eval.h)
    int init(int device, const char* conf, const mz_net_desc& desc, const float* weights, size_t count, Net* shared = nullptr, const mz_evaluator* ext = nullptr);
    // match play: two weight blobs of one descriptor, side A = (weights, count) of init, side B = these
    int initMatch(int device, const char* conf, const mz_net_desc& desc, const float* wa, size_t ca, const float* wb, size_t cb)
    {
        match_ = true;
        match_wb_ = wb;
        match_cb_ = cb;
        const int rc = init(device, conf, desc, wa, ca);
        match_wb_ = nullptr; // the caller's buffer: not kept
        return rc;
    }
    int matchStats(mz_match_stats* out) const
    {
        if (!match_) { setError("match_stats: the worker is not a match (mz_worker_create_match)"); return MZ_ERR_STATE; }
        *out = ms_;
        out->steps = match_t_;
        out->done = match_done_ ? 1 : 0;
        return MZ_OK;
    }
    int evaluatorBuffers(void** features, void** policy, void** logits, void** value) const;
    int evaluatorLanePolicy(float* out, int capacity);
    int command(const std::string& line);
    int loadModel(const std::string& path, const mz_net_desc& file_desc, const float* weights, size_t count);
    int setWeights(const float* w, size_t n)
    {
        if (match_) { return matchFixed("set_weights"); }
        pending_weights_.assign(w, w + n);
        return thinkReroot(-1, -1); // (mz_think_reuse_tree) a kept tree holds the old network's outputs
    }
    int runCycles(int n);
    int cyclesPerMove() const { return n_ + 1; }
    int numLanes() const { return plan_.lanes; }
    int popLine(char* buf, int cap);
    int waitLines();
    int peekRecord(int game, char* buf, int cap, const char* const* keys = nullptr, const char* const* values = nullptr, int ntags = 0);
    // the visited tree of a game as the pool holds it (tree_read.h): arrays, Tree::toString's SGF, and the node texts of ZeroActor::handleSearchDone
    int treeSnapshot(int g, TreeSnapshot* out);
    int treeString(int g, char* buf, int cap);
    int nodeInfo(int g, int which, char* buf, int cap);
    // per-actor stepping (mz_manual_step=true): BaseActor / ZeroActor surface (ref actor/base_actor.h:16-55, zero_actor.h:24-70)
    bool searchDone() const { return search_done_; }
    int searchAction(int g, int* action_id, int* player, int* resign) const;
    int actGame(int g, int action_id, int player);
    int resetSearchAll();
    int finishSearch();
    int resetGameAt(int g);
    int emitGame(int g);
    int envQuery(int g, int what, float* out) const;
    int actString(int g, const char* const* args, int nargs);
    int actionInfoHistory(int g, char* buf, int cap);
    int envFeatures(int g, int rotation, float* out, int capacity) const;
    int envLegalMask(int g, uint8_t* out, int capacity) const;
    int envSetTurn(int g, int player);
    int envResetSeed(int g, int seed);
    int envRotateAction(int g, int action_id, int rotation) const;
    mz_worker_stats stats_{};
    int thinkStats(uint64_t* steps, uint64_t* walks, uint64_t* queries) const
    {
        if (steps) { *steps = think_steps_; }
        if (walks) { *walks = think_walks_; }
        if (queries) { *queries = think_queries_; }
        return MZ_OK;
    }
    int thinkReuseStats(uint64_t* reroots, uint64_t* kept, uint64_t* kept_visits) const
    {
        if (reroots) { *reroots = reuse_reroots_; }
        if (kept) { *kept = reuse_kept_; }
        if (kept_visits) { *kept_visits = reuse_kept_visits_; }
        return MZ_OK;
    }
    int thinkSymmetryStats(long long* queries, long long* rows) const
    {
        if (queries) { *queries = static_cast<long long>(think_queries_); }
        if (rows) { *rows = static_cast<long long>(think_rows_); }
        return MZ_OK;
    }
    int getStats(mz_worker_stats* out)
    {
        *out = stats_;
        MZ_HIP(hipSetDevice(device_));
        for (auto& L : lanes_) {
            if (!L->net) { continue; } // external evaluator: no simulation kernels, nothing evaluated ahead
            for (Net* net : {L->net_b ? L->own_net.get() : L->net, L->net_b.get()}) { // (a match: both sides' networks)
                if (!net) { continue; }
                unsigned hits = 0, evals = 0, alt = 0;
                int rc = net->simPreStats(&hits, &evals, &alt);
                if (rc) { return rc; }
                out->pre_hits += hits; out->pre_evals += evals; out->pre_alt_hits += alt;
                out->pre_pair_launches += net->pre_pair_launches_;
            }
        }
        return MZ_OK;
    }
    Net& net0() { return *lanes_[0]->net; }
    // null: the worker runs on an external evaluator — or it is a match: Lane::net changes sides every step and the networks of a match are fixed,
    // so there is no handle through which mz_net_reload could reach one of them
    Net* netOrNull() { return match_ ? nullptr : lanes_[0]->net; }

private:
    // A lane = a contiguous slice of the games with its own device pool, network instance, HIP stream and staging.
    // Lanes are software-pipelined on the one host thread: while lane A's kernels (select / tower / heads) run, the
    // host builds candidates / leaf positions for lane B, and the two streams let the GPU overlap one lane's tower
    // (1 workgroup per sample: half the CUs at 128 games) with the other lane's tree kernels.  Results do not depend on
    // the lane count: the RNG-ordered serial section still visits the games in index order.
    struct Lane {
        int g0 = 0, n = 0;
        Net* net = nullptr;            // the lane's network: its own (own_net) or the caller's (mz_worker_create_shared)
        std::unique_ptr<Net> own_net;
        // match play: the lane holds BOTH sides' networks — own_net is side A's, net_b side B's — and `net` points at the one that searches this step.  Side B's
        // runs on the lane's stream (the pool's and the device rules' kernels are ordered with the network's on it); the stream it was created with goes with the lane
        std::unique_ptr<Net> net_b;
        hipStream_t net_b_stream = nullptr;
        int index = 0;
        Pool pool;
        std::unique_ptr<TreeReader> tree; // created with the lane's first read-out
        hipStream_t stream = nullptr;
        hipStream_t own_stream = nullptr; // external evaluator: there is no network whose stream the lane could share
        PinBuf<float> h_feat, h_out;
        PinBuf<uint8_t> h_raw;   // raw root observations (muzero_atari: bytes up, planes expanded on the device)
        DevBuf<uint8_t> d_raw;
        // incremental form: the device keeps the previous move's raw block (d_raw / d_raw2 alternate), the host sends the newest screen + 40 bytes per game
        PinBuf<uint8_t> h_new, h_meta;
        DevBuf<uint8_t> d_new, d_meta, d_raw2;
        int raw_cur = 0;          // which of (d_raw, d_raw2) holds the last uploaded / rebuilt block
        bool raw_have = false;    // ... and whether it holds one at all
        bool raw_incremental = false; // this root cycle: every game of the lane can be rebuilt from the previous block
        DevBuf<float> d_feat, d_out, d_hidden;
        Pool::View<float> h_policy, h_logit, h_value, h_reward, d_policy, d_logit, d_value, d_reward;
        DevBuf<int> d_src_idx, d_dst_idx, d_action_ids;
        int signal_seq = 0; // last completion signal queued on this lane's stream
        // device-resident leaf environment (AlphaZero Go): per-cycle rotations travel as a kernel argument
        GoDevice godev;
        RotPack rot{};
        int cycles_since_signal = 0;
        PinBuf<uint8_t> h_rot;   // per-game simulation kernel: rotations of a batch of cycles [cycle][game]
        DevBuf<uint8_t> d_rot;
        // MuZero simulation kernel: root planes (bit-packed), legal mask and player of every game, refreshed once per move
        PinBuf<uint32_t> h_rootfeat; DevBuf<uint32_t> d_rootfeat;
        PinBuf<unsigned long long> h_rootlegal; DevBuf<unsigned long long> d_rootlegal;
        PinBuf<int> h_rootturn; DevBuf<int> d_rootturn;
        bool rr_ahead = false;                // the root statistics of the finished search are already on their way (Pool::rootReadLaunch behind the move's last launch)
        PinBuf<unsigned> h_prestat;           // Gumbel rounds: the network's counters of leaves evaluated ahead, copied behind every move's launches (adaptRounds)
        PinBuf<int> h_gum; DevBuf<int> d_gum; // Gumbel state of every game (gumbel.h): the device runs the halving between simulations
        PinBuf<float> h_noise;   // Dirichlet noise of the root children drawn ahead of the launch [game][A]
        DevBuf<float> d_noise;
        // GPU time of the simulation-kernel launches (stats: ms_forward): one pair of events per part of a move's launch (runCyclesSim)
        static constexpr int kSimParts = 24; // parts a launch can be cut into (a Gumbel-round move of muzero_atari: one part per round that is evaluated ahead + the stretches between)
        int pre_epoch = 0;        // serial number of the current move's pre-evaluated leaves (mz_sim_rounds), 0: none
        hipEvent_t ev0[kSimParts] = {}, ev1[kSimParts] = {};
        hipStream_t up_stream = nullptr; // uploads of the draws for a later part while an earlier part runs on `stream`
        hipEvent_t ev_up = nullptr;
        int makeSimEvents()
        {
            for (int k = 0; k < kSimParts; ++k) { MZ_HIP(hipEventCreate(&ev0[k])); MZ_HIP(hipEventCreate(&ev1[k])); }
            MZ_HIP(hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking));
            MZ_HIP(hipEventCreateWithFlags(&ev_up, hipEventDisableTiming));
            return MZ_OK;
        }
        ~Lane()
        {
            for (int k = 0; k < kSimParts; ++k) { if (ev0[k]) { (void)hipEventDestroy(ev0[k]); } if (ev1[k]) { (void)hipEventDestroy(ev1[k]); } }
            if (ev_up) { (void)hipEventDestroy(ev_up); }
            if (up_stream) { (void)hipStreamDestroy(up_stream); }
            if (own_stream) { (void)hipStreamDestroy(own_stream); }
            if (net_b_stream) { (void)hipStreamDestroy(net_b_stream); }
        }
    };
    Lane& laneOf(int g) { return *lanes_[std::min(g / plan_.lane_size, plan_.lanes - 1)]; }
    int phase1(Lane& L, bool root_expansion, bool done, bool launch_select = true);
    int phase2(Lane& L);
    int phase2Resident(Lane& L);
    // external evaluator (ext_eval.h): the network step of the resident cycle is a hand-over to the caller's code and back
    std::unique_ptr<ExtEval> ext_;         // lane 0's (an external worker has one lane)
    bool external_ = false;
    mz_evaluator ext_ev_{};
    int feat_size_ = 0;                    // floats per sample of the feature planes: the network's, or the external evaluator's descriptor's
    std::string ext_failed_;               // forward() returned non-zero: the text every later run_cycles repeats
    int extRefusal() const;
    int extCheckDesc(const GameEnv& e) const;
    int runCyclesSim(int n);
    // batched think (actor_mcts_think_batch_size > 1 under mz_manual_step; think.h): a cycle is one STEP of every game whose search is not done
    int thinkB_ = 1;                       // the batch size in force (1: today's path, untouched)
    std::unique_ptr<ThinkDevice> think_;   // lane 0's (a think worker has one lane)
    std::vector<int> think_count_;         // root visits of every game (the games of a worker finish after different numbers of steps)
    std::vector<uint8_t> think_done_;
    std::vector<int> think_vl_child_;      // >= -1: the decision of game g sees one virtual loss on the root and on this root child (-1: on the root alone); -2: none
    uint64_t think_steps_ = 0, think_walks_ = 0, think_queries_ = 0;
    // mz_think_reuse_tree: mz_worker_act re-roots the game's tree at the move played (think_reroot_kernel) and the next search goes on from it
    bool think_reuse_ = false;
    std::vector<int> think_kept_;          // root visits of the tree game g keeps for its next search (0: none, reset_search clears as ever)
    std::vector<uint8_t> think_moved_;     // the tree of game g was re-rooted or cleared since its last decision: the chosen child is no longer a root child
    uint64_t reuse_reroots_ = 0, reuse_kept_ = 0, reuse_kept_visits_ = 0; // moves given to the re-root, those that kept a subtree, the visits of the kept roots
    // mz_think_symmetries: 8 = every query's leaf is evaluated under the eight symmetries of the board and averaged (think_sym_planes_kernel,
    // think_sym_reduce_kernel around the step's forward); the rotations thinkCycle draws are then drawn for the generator's sake alone
    int think_sym_ = 1;
    uint64_t think_rows_ = 0;              // network rows computed for the queries: think_sym_ per query
    int symRefusal(const char* where) const;
    int thinkReroot(int g, int action); // g < 0: every game; action -1 clears
    int reuseRefusal(const char* where) const;
    int thinkRefusal() const;
    int thinkCycle();
    int thinkReadRoots(Lane& L);
    void drawRootNoise(int g, std::vector<float>& noise);
    float vlOf(int g, int child) const { return (think_vl_child_.empty() || think_vl_child_[g] < -1) ? 0.0f : ((child < 0 || child == think_vl_child_[g]) ? 1.0f : 0.0f); }
    void drawCycles(int b0, int b1, int noise_row);
    void drawStream(int t, int b0, int b1, int noise_row);
    int uploadRoots(Lane& L);
    int cycle();
    int createActors();
    int resetAllSearches(const uint8_t* mask = nullptr);
    void resetGame(Game& g, Rng& rng);          // ZeroActor::reset (ref zero_actor.cpp:23-27)
    int rootPlayerFor(const Game& g) const { return g.env->numPlayers() == 2 ? 3 - g.env->turn() : g.env->turn(); }
    void buildCandidates(int g);
    void buildLeaf(int g);
    // per-move host logic on root statistics (rr_* mirrors)
    float normalizedMean(float reward, float mean, float count, int player, int g, float vl = 0.0f) const;
    int selectChildByMaxCount(int g) const;
    int selectChildBySoftmaxCount(int g, float temperature, float value_threshold = 0.1f);
    bool isResign(int g) const;
    std::string searchDistributionString(int g) const;
    std::string gumbelPolicyString(int g, int child_player) const;
    void gumbelSortByScore(int g);
    void gumbelSequentialHalving(int g);
    int decideAction(int g);
    void handleSearchDone(int g);
    void outputGame(Game& gm);
    std::pair<int, int> trainingDataRange(const Game& gm) const;
    // obs_raw != nullptr: the OBS tag is left as a one-byte placeholder and the observation bytes are returned for finishObservations()
    std::string record(const Game& gm, const ActionInfo& extra, std::string* obs_raw = nullptr) const;
    std::unique_ptr<ObsCompressor> obs_; // created with the first record that carries observations
    ActionInfo actionInfo(int g, int child_player) const;

    WorkerConfig cfg_;
    mz_net_desc desc_{};
    int device_ = 0, G_ = 0, A_ = 0, n_ = 0;
    std::vector<std::unique_ptr<Lane>> lanes_;
    std::unique_ptr<ThreadPool> threads_;
    std::vector<Game> games_;
    Rng main_rng_;
    // The slave threads' generators (ref actor_group.cpp:66-70: thread id seeds program_seed + id).  mz_rng_streams = 1 (default): every game draws from the
    // generator of slave thread 0 — the deterministic contract, and one of the schedules the reference's first-come-first-served hand-out of actors to threads
    // (actor_group.cpp:18-22) can produce.  mz_rng_streams = 0: as many generators as the reference has, zero_num_threads = T, the games statically partitioned
    // over them in contiguous blocks (streamOf) — another of those schedules (mz_rng_streams = S > 1: S generators whatever zero_num_threads says).  Every draw of game g comes from rngOf(g) in the reference's per-actor order; draws of different
    // streams are independent, so the long runs of draws (root noise, rotations: drawCycles) are made by the streams side by side on the pool's threads.
    std::vector<Rng> rngs_;
    int streams_ = 1;
    // the pool's size: zero_num_threads, never more than the CPUs we may burn
    int hostThreads() const { return std::max(1, std::min(cfg_.zero_num_threads, usableCpus() - 1)); }
    int streamOf(int g) const { return static_cast<int>(static_cast<long long>(g) * streams_ / G_); }
    Rng& rngOf(int g) { return rngs_[streamOf(g)]; }
    std::vector<std::vector<float>> stream_noise_;   // per stream: scratch of a noise draw
    bool running_ = false, pending_ = false;
    int sims_done_ = 0; // root visit count of every game (lock-step: identical for all games)
    int sim_pre_ = 0, sim_post_ = 0; // its value before / after the expand+backup of the current cycle
    std::deque<std::unique_ptr<OutLine>> lines_;
    std::vector<float> pending_weights_;
    // root statistics mirrors (valid after rootRead)
    std::vector<int> rr_nc_, rr_action_, rr_bsize_;
    std::vector<float> rr_count_, rr_mean_, rr_policy_, rr_logit_, rr_noise_, rr_value_, rr_reward_, rr_root_count_, rr_root_mean_, rr_root_value_,
        rr_lo_, rr_hi_;
    std::vector<uint8_t> noise_mask_;
    std::vector<float> noise_policy_, noise_logit_, noise_noise_;
    PhaseTrace trace_;
    int flipping_player_ = 2;
    struct DeferredInfo { int g, mover; size_t index; };
    // what the per-move host logic of one RNG stream's games leaves for the pool: with several streams (mz_rng_streams) the streams' blocks of games run side by
    // side on the pool's threads and their results are merged in stream order = game order (serialSection)
    struct StreamSink {
        uint64_t moves = 0, games = 0;
        std::vector<DeferredInfo> deferred;
        struct Line { std::unique_ptr<OutLine> line; std::string obs_raw; bool has_obs = false; };
        std::vector<Line> lines;
    };
    std::vector<StreamSink> sinks_;
    static thread_local StreamSink* tl_sink_; // the sink of the stream this thread is working for (nullptr: write through)
    void queueLine(std::unique_ptr<OutLine> line, std::string&& obs_raw, bool has_obs);
    void serialSection(Lane& L, bool want_noise, bool done, bool az);
    void serialGame(int g, bool want_noise, bool done, bool az, std::vector<float>& noise);
    std::vector<float> noise_scratch_;
    std::vector<DeferredInfo> deferred_; // record strings of the last move, built while the next launch runs
    void flushDeferred();
    struct Held { int action = -1, player = 0; bool resign = false; ActionInfo info; };
    std::vector<Held> held_;  // mz_manual_step: the decision of the completed search of every game
    bool search_done_ = false, stop_now_ = false;
    GumbelView gum_{};        // constants of the device-side Gumbel step (state pointer set per lane)
    bool root_host_pending_ = false; // plan_.sim_root_host: the root's outputs the next phase1 still has to turn into the root's children (host candidate lists)
    int syncGumbel(Lane& L, bool to_device);
    struct Round { int s0, R; float p_event = 0.0f; bool alt = false; }; // p_event: share of the recent moves in which a simulation of the round missed its leaf / took the second one
    std::vector<unsigned> prestat_prev_; // the counters as of the previous move (summed over the lanes)
    void adaptRounds();
    bool pairsUsable() // two workgroups per leaf (sim.hip sim_pre_pair_kernel_mz)
    {
        if (!(cfg_.mz_sim_round_pairs && plan_.lanes == 1 && net0().pairsAvailable())) { return false; }
        const int sharing = counted_device_ < 0 ? 1 : g_workers_on_device[counted_device_].load();
        if (sharing == 1) { return true; }
        if (!pairs_off_logged_) { // said once: otherwise nothing explains the slower rounds (an idle or not yet collected worker object on the device is enough)
            pairs_off_logged_ = true;
            fprintf(stderr, "[mzgpu] device %d carries %d workers of this process: sim_pre_pair_kernel_mz (two workgroups per leaf) stays off for this worker\n", device_, sharing);
        }
        return false;
    }
    bool pairs_off_logged_ = false;
    std::vector<Round> rounds_; // plan_.rounds as adaptRounds tunes them from move to move
    bool shared_net_ = false; // the network belongs to the caller (mz_worker_create_shared): load_model only renames, the caller reloads

    // How this worker runs: every execution choice, resolved in one place (resolvePlan) before anything that depends on it is allocated, and fixed afterwards.
    // None of it shows in a record.
    struct Plan {
        int lanes = 1, lane_size = 1;   // the games cut into `lanes` contiguous slices of lane_size (the last one may be shorter)
        bool feat_bits = false;         // AlphaZero leaves travel host->device as bit-packed planes (all board-game planes are 0/1)
        int raw_bytes = 0;              // > 0: root observations travel as bytes (GameEnv::rawFeatures) and are expanded on the device
        bool resident = false;          // AlphaZero: the whole cycle runs on the device (go_dev.hip): the host only does the RNG-ordered per-move logic
        bool sim_mz = false;            // MuZero on sim_kernel_mz (no device rules needed: the leaves have no environment)
        bool sim_kernel = false;        // whole runs of cycles are ONE launch of a per-game simulation kernel (sim.hip): resident with an instance, or sim_mz
        bool sim_root_host = false;     // muzero_atari on sim_kernel_mz: the root (96x96 representation) is evaluated by a lock-step cycle
        bool dev_gumbel = false;        // Gumbel root logic inside the simulation kernel
        bool defer_info = false;        // the record strings of a move are built while the next launch runs
        int slab_slots = 0;             // MuZero: hidden-state slots per game
        std::vector<Round> rounds;      // mz_sim_rounds: the rounds of a move whose leaves are evaluated ahead (first simulation, size), from the Gumbel schedule of (n, m)
        SimMzMode sim_mode;             // the MuZero simulation kernels' launch mode (launch arguments: the network may be shared with other workers)
        long split_min_draws = 32768;   // mz_sim_split: AlphaZero rotation draws a move needs before its launch gets a third part (MZ_SIM_SPLIT_MIN_DRAWS: tests, 0 = always)
    };
    Plan plan_;
    Plan resolvePlan(int lanes, const Net* asked = nullptr) const; // asked: the network whose kernels decide (nullptr: the first lane's)
    // ---- match play (mz_worker_create_match) ----
    bool match_ = false, match_done_ = false;
    const float* match_wb_ = nullptr;  // side B's parameters while init runs
    size_t match_cb_ = 0;
    uint64_t match_t_ = 0;             // the step counter t: steps (one move of every game each) since `start`
    mz_match_stats ms_{};
    int matchRefusal() const;
    int matchFixed(const char* what) const { setError("%s: the networks of a match are fixed when it is created (a new match is a new worker)", what); return MZ_ERR_STATE; }
    const std::string& matchPrecision(int side) const
    {
        const std::string& p = side ? cfg_.mz_match_precision_b : cfg_.mz_match_precision_a;
        return p.empty() ? cfg_.mz_nn_precision : p;
    }
    const std::string& matchName(int side) const { return side ? cfg_.mz_match_name_b : cfg_.mz_match_name_a; }
    int matchBeginStep(Lane& L, uint64_t t);
    void matchAfterMoves(Lane& L);
    bool matchOver() const { return ms_.games_finished >= uint64_t(cfg_.mz_match_games); }
    int addLane(Net* shared, const float* weights, size_t count);
    int allocLane(int l, const mz_search_cfg& sc);
};

// ------------------------------------------------------------------------------------------------
int Worker::init(int device, const char* conf, const mz_net_desc& desc, const float* weights, size_t count, Net* shared, const mz_evaluator* ext)
{
    if (!conf || !cfg_.loadFromString(conf)) { return MZ_ERR_ARG; }
    desc_ = desc;
    device_ = device;
    external_ = ext != nullptr;
    if (external_) { ext_ev_ = *ext; }
    if (device >= 0 && device < 64) { counted_device_ = device; g_workers_on_device[device].fetch_add(1); }
    if (cfg_.mz_think_reuse_tree && (external_ || match_)) { return reuseRefusal(external_ ? "external" : "match"); }
    if (cfg_.mz_think_symmetries != 1 && (external_ || match_)) { return symRefusal(external_ ? "external" : "match"); }
    if (external_) { int rx = extRefusal(); if (rx) { return rx; } }
    if (match_) { int rm = matchRefusal(); if (rm) { return rm; } }
    if (cfg_.nn_type_name == "muzero" && desc.type == 0) { setError("nn_type_name=muzero but the network descriptor is alphazero"); return MZ_ERR_ARG; }
    if (gameFromName(cfg_.env_game.c_str()) == kHavannah && (cfg_.nn_type_name != "alphazero" || desc.type != 0)) { // ref havannah.cpp:233-236: getActionFeatures throws
        setError("env_game=havannah has no action features: a MuZero network cannot play it (nn_type_name=alphazero only, ref havannah.cpp:233-236)");
        return MZ_ERR_ARG;
    }
    if (cfg_.zero_num_parallel_games <= 0 || cfg_.actor_num_simulation <= 0) { setError("zero_num_parallel_games and actor_num_simulation must be > 0"); return MZ_ERR_ARG; }
    if (cfg_.zero_num_parallel_games > 4096) { setError("zero_num_parallel_games > 4096 (ref alphazero_network.h:120 kReserved_batch_size)"); return MZ_ERR_ARG; }
    if (cfg_.mz_nn_precision != "f32" && cfg_.mz_nn_precision != "bf16x3") { setError("mz_nn_precision '%s' unknown (f32 | bf16x3)", cfg_.mz_nn_precision.c_str()); return MZ_ERR_ARG; }
    if (shared && shared->device_ != device) { setError("worker: the shared network lives on device %d, the worker on %d", shared->device_, device); return MZ_ERR_ARG; }
    thinkB_ = cfg_.mz_manual_step ? std::max(1, cfg_.actor_mcts_think_batch_size) : 1; // without mz_manual_step the key stays ignored, as ActorGroup never uses it
    if (thinkB_ > 1) { int rt = thinkRefusal(); if (rt) { return rt; } }
    if (cfg_.mz_think_reuse_tree) { int rt = reuseRefusal(nullptr); if (rt) { return rt; } }
    think_reuse_ = cfg_.mz_think_reuse_tree;
    if (cfg_.mz_think_symmetries != 1) { int rt = symRefusal(nullptr); if (rt) { return rt; } }
    think_sym_ = cfg_.mz_think_symmetries;
    G_ = cfg_.zero_num_parallel_games;
    A_ = desc.action_size;
    n_ = cfg_.actor_num_simulation;
    flipping_player_ = (cfg_.actor_mcts_value_flipping_player == 'B' || cfg_.actor_mcts_value_flipping_player == 'b') ? 1
                       : (cfg_.actor_mcts_value_flipping_player == 'W' || cfg_.actor_mcts_value_flipping_player == 'w') ? 2 : 3;
    shared_net_ = shared != nullptr;
    // the first lane's network: the plan asks it which kernels the shape has (at its precision: hasSimKernelWide depends on it)
    int rc = addLane(shared, weights, count);
    if (rc) { return rc; }
    feat_size_ = external_ ? desc.num_input_channels * desc.input_channel_height * desc.input_channel_width : net0().featSize();
    // the pool spins: never more spinners than CPUs the container may use, minus one for the HIP runtime's helper threads
    threads_ = std::make_unique<ThreadPool>(hostThreads(), cfg_.mz_cpu_base);
    const size_t GA = size_t(G_) * A_;
    rr_nc_.resize(G_); rr_action_.resize(GA); rr_bsize_.resize(G_);
    for (auto* v : {&rr_count_, &rr_mean_, &rr_policy_, &rr_logit_, &rr_noise_, &rr_value_, &rr_reward_}) { v->resize(GA); }
    for (auto* v : {&rr_root_count_, &rr_root_mean_, &rr_root_value_, &rr_lo_, &rr_hi_}) { v->resize(G_); }
    noise_mask_.assign(G_, 1);
    held_.assign(G_, Held());
    noise_policy_.resize(GA); noise_logit_.resize(GA); noise_noise_.resize(GA);
    if ((rc = createActors())) { return rc; }
    if (think_sym_ == 8) { // the eight views of a leaf have to be eight different maps: decided from the game's own tables, not from its name
        const RotationTables* rt = games_[0].env->rot();
        bool distinct = rt != nullptr;
        for (int a = 0; a < 8 && distinct; ++a) {
            for (int b = a + 1; b < 8 && distinct; ++b) { distinct = rt->inv[a] != rt->inv[b] && rt->fwd[a] != rt->fwd[b]; }
        }
        if (!distinct) {
            setError("mz_think_symmetries=8 with env_game=%s: the game has no eight symmetries (its rotation tables are not eight different maps), so the eight views of a leaf would be one",
                     cfg_.env_game.c_str());
            return MZ_ERR_ARG;
        }
    }
    plan_ = resolvePlan(match_ ? 2 : std::max(1, cfg_.mz_pipeline_lanes));
    if (match_) {
        // one plan serves both lanes and every step: the two sides' networks (the first lane holds both) must ask for the same one
        const Plan pb = resolvePlan(2, lanes_[0]->net_b.get());
        if (pb.resident != plan_.resident || pb.sim_mz != plan_.sim_mz || pb.sim_kernel != plan_.sim_kernel || pb.sim_root_host != plan_.sim_root_host ||
            pb.dev_gumbel != plan_.dev_gumbel || pb.feat_bits != plan_.feat_bits || pb.slab_slots != plan_.slab_slots || pb.rounds.size() != plan_.rounds.size() ||
            pb.sim_mode.cluster != plan_.sim_mode.cluster || pb.sim_mode.rounds != plan_.sim_mode.rounds || pb.sim_mode.alt_base != plan_.sim_mode.alt_base) {
            setError("mz_match_precision_a=%s / mz_match_precision_b=%s: the two sides of a match resolve to different execution plans (%s against %s); "
                     "set mz_sim_kernel=false to play both in the lock-step mode", matchPrecision(0).c_str(), matchPrecision(1).c_str(),
                     plan_.sim_kernel ? "a simulation kernel" : "lock-step", pb.sim_kernel ? "a simulation kernel" : "lock-step");
            return MZ_ERR_ARG;
        }
    }
    while (int(lanes_.size()) < plan_.lanes) { if ((rc = addLane(shared, weights, count))) { return rc; } }
    mz_search_cfg sc{};
    sc.num_simulation = n_;
    sc.puct_base = cfg_.actor_mcts_puct_base;
    sc.puct_init = cfg_.actor_mcts_puct_init;
    sc.reward_discount = cfg_.actor_mcts_reward_discount;
    sc.value_rescale = cfg_.actor_mcts_value_rescale;
    sc.flipping_player = flipping_player_;
    sc.atari_init_q = cfg_.atari_init_q;
    if (external_ && !plan_.resident) { // (extRefusal and extCheckDesc name every way there: kept for the plan's own conditions)
        setError("external evaluator: this configuration does not run on the device rules (the resident plan), which the hand-over needs");
        return MZ_ERR_ARG;
    }
    for (int l = 0; l < plan_.lanes; ++l) { if ((rc = allocLane(l, sc))) { return rc; } }
    if (external_) {
        Lane& L = *lanes_[0];
        if (!createExtEval) { setError("external evaluator: this build has no device code for the hand-over (ext_eval.hip is not linked)"); return MZ_ERR_DEVICE; }
        ext_.reset(createExtEval());
        const GoDevView& gv = L.godev.v_;
        if ((rc = ext_->init(device_, L.stream, ExtEvalShape{L.n, gv.channels, gv.P, gv.W32, A_}, ext_ev_))) { return rc; }
    }
    if (plan_.dev_gumbel) { // the constants of gumbel_zero.cpp:101,110 in the host's double arithmetic
        const int m = cfg_.actor_gumbel_sample_size;
        gum_.sample_size = m;
        gum_.sigma_visit_c = cfg_.actor_gumbel_sigma_visit_c;
        gum_.sigma_scale_c = cfg_.actor_gumbel_sigma_scale_c;
        gum_.budget0 = static_cast<int>(std::max(1.0, std::floor(n_ / (std::log2(m) * m))));
        gum_.num_simulation = n_;
        gum_.log2_m = std::log2(m);
    }
    rounds_ = plan_.rounds;
    if (match_) { // the first G games are counted (mz_match_games >= G) and start at step 0: lane h's first player is side h
        for (int g = 0; g < G_; ++g) {
            games_[g].m_serial = g;
            games_[g].m_t0 = 0;
            games_[g].m_first_side = laneOf(g).index & 1;
        }
        ms_.games_started = uint64_t(G_);
    }
    if (thinkB_ > 1) {
        if (!plan_.resident) { setError("actor_mcts_think_batch_size=%d: the batched think runs on the device rules, which this game or pool size does not have", thinkB_); return MZ_ERR_ARG; }
        Lane& L = *lanes_[0];
        if (!createThinkDevice) { setError("actor_mcts_think_batch_size=%d: this build has no device code for the batched think", thinkB_); return MZ_ERR_DEVICE; }
        think_.reset(createThinkDevice());
        if ((rc = think_->init(device_, L.stream, L.pool, L.godev.v_, thinkB_, sc, think_reuse_, think_sym_))) { return rc; }
        think_kept_.assign(G_, 0);
        think_moved_.assign(G_, 0);
        think_count_.assign(G_, 0);
        think_done_.assign(G_, 0);
        think_vl_child_.assign(G_, -2);
    }
    return resetAllSearches();
}

// mz_worker_create_external: what the hand-over does not cover is refused by name when the worker is created
int Worker::extRefusal() const
{
    if (!ext_ev_.forward) { setError("external evaluator: forward is NULL"); return MZ_ERR_ARG; }
    if (desc_.type != 0) { setError("desc.type=%d: an external evaluator is an AlphaZero network (type 0; a MuZero one needs the caller to own the hidden states)", desc_.type); return MZ_ERR_ARG; }
    if (cfg_.nn_type_name != "alphazero") { setError("nn_type_name=%s: an external evaluator is an AlphaZero network (nn_type_name=alphazero)", cfg_.nn_type_name.c_str()); return MZ_ERR_ARG; }
    if (gameFromName(cfg_.env_game.c_str()) == kNoDeviceGame) { setError("env_game=%s has no rules on the device, which the external evaluator's hand-over needs", cfg_.env_game.c_str()); return MZ_ERR_ARG; }
    if (!cfg_.mz_device_env) { setError("mz_device_env=false: the external evaluator is handed the leaves of the device rules"); return MZ_ERR_ARG; }
    if (cfg_.zero_num_parallel_games > kRotPackGames) { setError("zero_num_parallel_games=%d: an external evaluator has one lane of at most %d games", cfg_.zero_num_parallel_games, kRotPackGames); return MZ_ERR_ARG; }
    if (cfg_.mz_pipeline_lanes >= 2) { setError("mz_pipeline_lanes=%d: an external evaluator is called once per cycle, for one lane", cfg_.mz_pipeline_lanes); return MZ_ERR_ARG; }
    if (cfg_.actor_mcts_think_batch_size > 1) { setError("actor_mcts_think_batch_size=%d: the batched think does not run on an external evaluator", cfg_.actor_mcts_think_batch_size); return MZ_ERR_ARG; }
    if (cfg_.mz_nn_precision != "f32") { setError("mz_nn_precision=%s: with an external evaluator the precision is the caller's business (leave the key at f32)", cfg_.mz_nn_precision.c_str()); return MZ_ERR_ARG; }
    return MZ_OK;
}

// mz_worker_create_match: what the schedule of a match (two lanes, one move of every game per step, strict alternation) does not cover is refused by name
// when the worker is created
int Worker::matchRefusal() const
{
    const int G = cfg_.zero_num_parallel_games, N = cfg_.mz_match_games;
    if (G < 2 || (G & 1)) { setError("zero_num_parallel_games=%d: a match plays two lanes of G / 2 games each (an even number, at least 2)", G); return MZ_ERR_ARG; }
    if (N < G) { setError("mz_match_games=%d: a match counts at least as many games as it plays side by side (zero_num_parallel_games=%d)", N, G); return MZ_ERR_ARG; }
    if (cfg_.env_game == "atari") { setError("env_game=atari: a match needs a game of two players"); return MZ_ERR_ARG; }
    if (cfg_.mz_manual_step) { setError("mz_manual_step=true: a match plays on its own, step by step for both sides"); return MZ_ERR_ARG; }
    if (cfg_.actor_mcts_think_batch_size > 1) { setError("actor_mcts_think_batch_size=%d: a match searches one simulation at a time (the batched think has one lane)", cfg_.actor_mcts_think_batch_size); return MZ_ERR_ARG; }
    if (cfg_.zero_actor_intermediate_sequence_length > 0) {
        setError("zero_actor_intermediate_sequence_length=%d: a match prints whole games, one line each", cfg_.zero_actor_intermediate_sequence_length);
        return MZ_ERR_ARG;
    }
    for (int side = 0; side < 2; ++side) {
        const std::string& p = matchPrecision(side);
        if (p != "f32" && p != "bf16x3") { setError("mz_match_precision_%c '%s' unknown (f32 | bf16x3): a match runs each side at one of the two", side ? 'b' : 'a', p.c_str()); return MZ_ERR_ARG; }
    }
    if (!match_wb_) { setError("match: side B has no parameters"); return MZ_ERR_ARG; }
    return MZ_OK;
}

// The schedule at a move boundary, before the step's first launch: in step t lane h is searched by side (h + t) mod 2, and every game of the lane must have
// that side to move — a game that started at step t0 has had t - t0 steps (a move each), so its first player (Black) moves when t - t0 is even.
int Worker::matchBeginStep(Lane& L, uint64_t t)
{
    const int side = static_cast<int>((uint64_t(L.index) + t) & 1);
    L.net = side ? L.net_b.get() : L.own_net.get();
    for (int g = L.g0; g < L.g0 + L.n; ++g) {
        const Game& gm = games_[g];
        const int expect = ((t - gm.m_t0) & 1) ? 2 : 1;
        if (gm.env->turn() != expect) {
            setError("match: game %d of lane %d has player %d to move at step %llu, %llu steps after its start: turn disagrees with the schedule's parity (player %d), "
                     "so the lane's games no longer share their side to move", g, L.index, gm.env->turn(), (unsigned long long)t, (unsigned long long)(t - gm.m_t0), expect);
            return MZ_ERR_STATE;
        }
    }
    return MZ_OK;
}

// What the step's moves did, in slot order (the host section that made them may have run the RNG streams side by side): the tally of the counted games that
// ended, and for every slot that freed up the game that starts in it at step t + 1 — the next serial number while fewer than mz_match_games have started,
// else an uncounted filler; its first player is side (h + t + 1) mod 2, the side that searches the lane in that step.
void Worker::matchAfterMoves(Lane& L)
{
    for (int g = L.g0; g < L.g0 + L.n; ++g) {
        Game& gm = games_[g];
        if (gm.m_serial >= 0 && gm.m_acted) { ++ms_.moves; }
        if (gm.m_ended) {
            if (gm.m_serial >= 0) {
                const int first = gm.m_score > 0 ? 0 : (gm.m_score < 0 ? 2 : 1); // win / draw / loss of the first player (Black)
                if (gm.m_first_side == 0) { ++ms_.a_first[first]; } else { ++ms_.a_second[2 - first]; }
                ++ms_.games_finished;
                if (gm.m_resigned) { ++ms_.resignations; }
            }
            gm.m_t0 = match_t_ + 1;
            gm.m_first_side = static_cast<int>((uint64_t(L.index) + gm.m_t0) & 1);
            if (ms_.games_started < uint64_t(cfg_.mz_match_games)) { gm.m_serial = static_cast<int>(ms_.games_started++); }
            else { gm.m_serial = -1; ++ms_.filler_games; }
        }
        gm.m_acted = gm.m_ended = gm.m_resigned = false;
    }
}

// the four numbers of the descriptor an external evaluator is created with, against the game's engine
int Worker::extCheckDesc(const GameEnv& e) const
{
    if (!e.hasDeviceTwin()) { setError("env_game=%s at env_board_size=%d has no rules on the device, which the external evaluator's hand-over needs", cfg_.env_game.c_str(), cfg_.env_board_size); return MZ_ERR_ARG; }
    const int planes = gameChannels(e.deviceKind());
    if (desc_.num_input_channels != planes) { setError("external evaluator: desc.num_input_channels=%d, but %s has %d feature planes", desc_.num_input_channels, e.name().c_str(), planes); return MZ_ERR_ARG; }
    if (desc_.input_channel_height != e.boardSize() || desc_.input_channel_width != e.boardSize()) {
        setError("external evaluator: desc.input_channel_height x width = %d x %d, but the planes of %s are %d x %d", desc_.input_channel_height, desc_.input_channel_width,
                 e.name().c_str(), e.boardSize(), e.boardSize());
        return MZ_ERR_ARG;
    }
    if (desc_.action_size != e.policySize()) { setError("external evaluator: desc.action_size=%d, but the policy of %s has %d actions", desc_.action_size, e.name().c_str(), e.policySize()); return MZ_ERR_ARG; }
    return MZ_OK;
}

// mz_think_reuse_tree=true: the option belongs to the batched think; where that does not run, or where a root that is already expanded would need a rule
// of its own, it is refused by name when the worker is created
int Worker::reuseRefusal(const char* where) const
{
    if (where && where[0] == 'e') { setError("mz_think_reuse_tree=true: an external evaluator does not run the batched think, whose trees the option keeps"); return MZ_ERR_ARG; }
    if (where) { setError("mz_think_reuse_tree=true: a match plays on its own, one simulation at a time (the option keeps the trees of the batched think)"); return MZ_ERR_ARG; }
    if (!cfg_.mz_manual_step) { setError("mz_think_reuse_tree=true without mz_manual_step=true: the tree is kept across mz_worker_act, which only a manually stepped worker takes"); return MZ_ERR_ARG; }
    if (thinkB_ < 2) { setError("mz_think_reuse_tree=true with actor_mcts_think_batch_size=%d: the option keeps the trees of the batched think (a batch size of 2 to %d)", cfg_.actor_mcts_think_batch_size, kThinkMaxBatch); return MZ_ERR_ARG; }
    if (cfg_.actor_use_dirichlet_noise) { setError("mz_think_reuse_tree=true with actor_use_dirichlet_noise=true: noise on a root that is already expanded needs a rule of its own"); return MZ_ERR_ARG; }
    if (cfg_.actor_use_gumbel_noise) { setError("mz_think_reuse_tree=true with actor_use_gumbel_noise=true: noise on a root that is already expanded needs a rule of its own"); return MZ_ERR_ARG; }
    return MZ_OK;
}

// mz_think_symmetries=8: the averaging is a part of the batched think's step; where that does not run it is refused by name when the worker is created (the
// game's own refusal, which needs the rotation tables, follows createActors in init)
int Worker::symRefusal(const char* where) const
{
    const int s = cfg_.mz_think_symmetries;
    if (where && where[0] == 'e') { setError("mz_think_symmetries=%d: an external evaluator does not run the batched think, whose leaves the key evaluates under eight symmetries", s); return MZ_ERR_ARG; }
    if (where) { setError("mz_think_symmetries=%d: a match plays on its own, one simulation at a time (the key belongs to the batched think)", s); return MZ_ERR_ARG; }
    if (s != 8) { setError("mz_think_symmetries=%d: 1 (one view per leaf) or 8 (all eight symmetries of the board)", s); return MZ_ERR_ARG; }
    if (!cfg_.mz_manual_step) { setError("mz_think_symmetries=8 without mz_manual_step=true: the key belongs to the batched think, which only a manually stepped worker runs"); return MZ_ERR_ARG; }
    if (thinkB_ < 2) { setError("mz_think_symmetries=8 with actor_mcts_think_batch_size=%d: the key belongs to the batched think (a batch size of 2 to %d)", cfg_.actor_mcts_think_batch_size, kThinkMaxBatch); return MZ_ERR_ARG; }
    return MZ_OK;
}

// actor_mcts_think_batch_size > 1: what the batched think does not cover is refused by name when the worker is created (documented differences)
int Worker::thinkRefusal() const
{
    const int B = thinkB_;
    if (B > kThinkMaxBatch) { setError("actor_mcts_think_batch_size=%d: at most %d walks per step", B, kThinkMaxBatch); return MZ_ERR_ARG; }
    if (desc_.type != 0 || cfg_.nn_type_name != "alphazero") { setError("actor_mcts_think_batch_size=%d: the batched think searches AlphaZero networks only (a MuZero network's step is not built)", B); return MZ_ERR_ARG; }
    if (cfg_.actor_use_gumbel) { setError("actor_mcts_think_batch_size=%d with actor_use_gumbel=true: the batched think has a PUCT root only", B); return MZ_ERR_ARG; }
    if (!cfg_.mz_device_env) { setError("actor_mcts_think_batch_size=%d with mz_device_env=false: the batched think runs on the device rules", B); return MZ_ERR_ARG; }
    if (cfg_.actor_mcts_value_rescale) { setError("actor_mcts_think_batch_size=%d with actor_mcts_value_rescale=true: the batched think keeps no value bounds (board games do not rescale)", B); return MZ_ERR_ARG; }
    return MZ_OK;
}

// Every execution choice of the worker, from the configuration, the descriptor, the game, the first lane's network (which kernels its shape has), the pool's
// size and whether the network is shared.  Pure — nothing is allocated — so the automatic lane count can resolve the plan for one lane and then for two.
Worker::Plan Worker::resolvePlan(int lanes, const Net* asked) const
{
    Plan p;
    const GameEnv& e = *games_[0].env;
    if (external_) { // no network to ask: one lane on the device rules, lock-step, the host runs the Gumbel root
        p.lane_size = G_;
        p.sim_mode.cluster = false;
        p.feat_bits = true;
        p.resident = cfg_.mz_device_env && e.hasDeviceTwin() && G_ <= kRotPackGames;
        return p;
    }
    const Net& net = asked ? *asked : *lanes_[0]->net;
    p.lanes = (G_ < 2 * lanes || shared_net_ || thinkB_ > 1) ? 1 : lanes; // a shared network has one stream: one lane; so has the batched think
    if (match_) { p.lanes = 2; } // a match is two lanes of G / 2 games, down to one game each
    p.lane_size = (G_ + p.lanes - 1) / p.lanes;
    p.sim_mode.cluster = cfg_.mz_sim_cluster && p.lanes == 1; // two lanes = two concurrent cooperative launches: not with clusters that wait for each other
    // AlphaZero board games: every plane is 0 / 1, so leaves reach the network bit-packed whatever kernels serve its shape — the fused towers stage the bits
    // themselves, the run-time-shaped per-layer kernels behind every other shape get them unpacked first (Net::runTrunk).  (Until round 6 this was tied to
    // hasFusedTower(), which also kept the device rules — resident below — away from every shape on conv3x3_band: a host hop per lock-step cycle.)
    p.feat_bits = desc_.type == 0;
    p.raw_bytes = (desc_.type == 2 && cfg_.mz_raw_observations) ? e.rawFeatureBytes() : 0;
    const bool gumbel_fits = !cfg_.actor_use_gumbel || (cfg_.actor_gumbel_sample_size >= 2 && cfg_.actor_gumbel_sample_size <= kGumbelMaxSample);
    p.resident = cfg_.mz_device_env && desc_.type == 0 && e.hasDeviceTwin() && p.lane_size <= kRotPackGames;
    p.sim_mz = cfg_.mz_sim_kernel && (desc_.type == 1 || desc_.type == 2) && net.hasSimKernelMz(n_) && gumbel_fits;
    p.sim_kernel = p.sim_mz || (p.resident && cfg_.mz_sim_kernel && thinkB_ == 1 && net.hasSimKernel(e.boardSize(), e.deviceKind(), n_) && gumbel_fits);
    p.sim_root_host = p.sim_mz && desc_.type == 2;
    p.dev_gumbel = p.sim_kernel && cfg_.actor_use_gumbel;
    p.defer_info = p.sim_kernel && !cfg_.mz_manual_step;
    // hidden-state slab: one slot per expanded node; with Gumbel rounds on muzero_atari a second bank for the rounds' second expected leaves
    if (desc_.type >= 1) { p.slab_slots = (n_ + 1) * ((desc_.type == 2 && cfg_.actor_use_gumbel && cfg_.mz_sim_rounds && cfg_.mz_sim_round_alt) ? 2 : 1); }
    if (p.sim_mz && p.dev_gumbel && (desc_.type == 2 || (desc_.type == 1 && cfg_.mz_sim_rounds_board && net.hasPreBoard())) && cfg_.mz_sim_rounds && cfg_.mz_sim_split) {
        // The visiting order of a Gumbel root is a function of the visit COUNTS alone (ref gumbel_zero.cpp:74-119: fewest visits first, halving when every
        // candidate has reached the budget): with m sampled children the simulations of a move fall into rounds in which every remaining candidate is visited
        // once — m, m/2, ... — e.g. n = 50, m = 16: 16, 8, 4, 4, 4, 2 x 7.  The rounds of >= kMinRound simulations are evaluated ahead (sim.hip
        // sim_pre_kernel_mz); a root with fewer than m children follows another schedule: its entries simply do not match and its simulations evaluate their
        // own leaves.
        const int kMinRound = std::max(1, cfg_.mz_sim_round_min);
        const int n = n_, m = cfg_.actor_gumbel_sample_size;
        if (m >= 2 && m <= kGumbelMaxSample && A_ >= m) {
            std::vector<int> cnt(m, 0);
            int ncand = m, sample = m;
            int budget = static_cast<int>(std::max(1.0, std::floor(n / (std::log2(m) * m))));
            int s = 1;
            while (s <= n) {
                if (s > 1) { // the step before simulation s (gumbel_zero.cpp:104-118)
                    bool all = true;
                    for (int i = 0; i < ncand; ++i) { if (cnt[i] < budget) { all = false; break; } }
                    if (all) {
                        const int next_budget = static_cast<int>(std::floor(n / (std::log2(m) * sample / 2)));
                        if (next_budget > 0 && sample > 2) {
                            sample /= 2;
                            if (ncand > sample) { ncand = sample; } // (which ones survive does not matter here: their counts are equal)
                            budget = cnt[0] + next_budget;
                        }
                    }
                }
                // a round: every candidate with the minimum count once
                int mn = cnt[0];
                for (int i = 1; i < ncand; ++i) { mn = std::min(mn, cnt[i]); }
                int R = 0;
                for (int i = 0; i < ncand; ++i) { if (cnt[i] == mn) { ++cnt[i]; ++R; } }
                R = std::min(R, n - s + 1);
                if (R >= kMinRound) { p.rounds.push_back({s, R}); p.rounds.back().alt = 2 * G_ * R <= net.cuCount(); } // (the second leaves from the first move on where they fit: adaptRounds takes them away where they are not used)
                s += R;
            }
        }
        int covered = 0;
        for (const Round& rd : p.rounds) { covered += rd.R; }
        p.sim_mode.rounds = !p.rounds.empty();
        p.sim_mode.alt_base = (!p.rounds.empty() && p.slab_slots == 2 * (n_ + 1)) ? n_ + 1 : 0;
        // every simulation of a move has its leaf evaluated ahead: what is left for the simulation kernel is the tree work of one wave per game, which one
        // workgroup per game does with less overhead than a cluster of four (no command / result exchange, no cooperative launch): 616 -> 656 k leaf-evals/s
        if (covered == n_) { p.sim_mode.cluster = false; }
    }
    if (const char* md = getenv("MZ_SIM_SPLIT_MIN_DRAWS")) { p.split_min_draws = atol(md); }
    // mz_pipeline_lanes = 0 (automatic): a pool that plays in the lock-step mode with the device rules — a shape without a simulation-kernel instance — and whose
    // cycle is dominated by long convolution kernels runs faster as TWO lanes on two streams: one lane's single-wave tree kernels (select, leaf, candidates, expand:
    // ~0.3 ms per cycle with 255 CUs idle) run under the other lane's convolutions.  Measured (profiles/r06_lockstep_lanes.json): 19x19 6b x 128, 256 games, 331 GFLOP
    // per cycle: 64.1 -> 67.1 k leaf-evals/s; 13x13 6b x 96, 73 GFLOP per cycle: 182 -> 167 k (its convolutions at 128 samples no longer fill the chip) — hence the bound.
    if (cfg_.mz_pipeline_lanes == 0 && p.lanes == 1 && !shared_net_ && thinkB_ == 1 && p.resident && !p.sim_kernel && G_ >= 64) {
        const double P = double(desc_.hidden_channel_height) * desc_.hidden_channel_width, C = desc_.num_hidden_channels;
        const double conv_flops = 2.0 * 9.0 * P * (double(desc_.num_input_channels) * C + 2.0 * desc_.num_blocks * C * C);
        if (double(G_) * conv_flops >= 2.0e11) { return resolvePlan(2); }
    }
    return p;
}

// A lane's network: the caller's (then the only lane; it keeps the precision its owner chose with mz_net_set_precision) or an instance of its own
int Worker::addLane(Net* shared, const float* weights, size_t count)
{
    auto L = std::make_unique<Lane>();
    if (external_) { // no network: a stream of the lane's own
        int count_dev = 0;
        if (hipGetDeviceCount(&count_dev) != hipSuccess || device_ < 0 || device_ >= count_dev) {
            (void)hipGetLastError();
            setError("no such GPU: device %d of %d (libmzgpu has no CPU path)", device_, count_dev);
            return MZ_ERR_DEVICE;
        }
        MZ_HIP(hipSetDevice(device_));
        MZ_HIP(hipStreamCreateWithFlags(&L->own_stream, hipStreamNonBlocking));
        L->stream = L->own_stream;
        lanes_.push_back(std::move(L));
        return MZ_OK;
    }
    if (shared) {
        L->net = shared;
    } else {
        L->own_net = std::make_unique<Net>();
        L->net = L->own_net.get();
        int rc = L->net->init(device_, desc_, weights, count);
        if (!rc) { rc = L->net->setPrecision((match_ ? matchPrecision(0) : cfg_.mz_nn_precision) == "bf16x3" ? 1 : 0); }
        if (rc) { return rc; }
        if (match_) { // side B's network beside side A's, on the same stream
            L->net_b = std::make_unique<Net>();
            rc = L->net_b->init(device_, desc_, match_wb_, match_cb_);
            if (!rc) { rc = L->net_b->setPrecision(matchPrecision(1) == "bf16x3" ? 1 : 0); }
            if (rc) { return rc; }
            MZ_HIP(hipStreamSynchronize(L->net_b->stream_));
            if (L->net_b->own_stream_) { L->net_b_stream = L->net_b->stream_; L->net_b->own_stream_ = false; }
            L->net_b->stream_ = L->net->stream_;
        }
    }
    L->index = static_cast<int>(lanes_.size());
    L->stream = L->net->stream_;
    lanes_.push_back(std::move(L));
    return MZ_OK;
}

// Lane l's slice of the games, device pool and staging, as the plan asks for them
int Worker::allocLane(int l, const mz_search_cfg& sc)
{
    Lane& L = *lanes_[l];
    L.g0 = l * plan_.lane_size;
    L.n = std::min(plan_.lane_size, G_ - L.g0);
    // ref actor_group.cpp:183: tree_node_size = (n + 1) * action_size; tree.h:66: 1 + tree_node_size nodes
    int rc = L.pool.init(device_, L.n, 1 + (n_ + 1) * A_, A_, sc, L.stream);
    if (rc) { return rc; }
    // kernels talk to the pinned staging directly: no memcpy operations on the per-cycle path (the device rules: nobody on the host reads the paths)
    if (cfg_.mz_zero_copy & 1) { L.pool.zero_copy_ = true; }
    if ((cfg_.mz_zero_copy & 2) && !plan_.resident) {
        L.pool.v_.host_path_len = L.pool.h_path_len_.p;
        L.pool.v_.host_path_action = L.pool.h_path_action_.p;
    }
    const size_t n = L.n, GA = n * A_, feat = n * feat_size_, rb = plan_.raw_bytes, sims = n_ + 1;
#define WALLOC(b, k) \
    if (!(b).alloc(k)) { setError("worker: allocation failed (%s)", #b); return MZ_ERR_DEVICE; }
    WALLOC(L.h_feat, feat); WALLOC(L.d_feat, feat); WALLOC(L.h_out, 2 * GA + 2 * n); WALLOC(L.d_out, 2 * GA + 2 * n);
    L.h_policy = {L.h_out.p, GA}; L.h_logit = {L.h_out.p + GA, GA}; L.h_value = {L.h_out.p + 2 * GA, n}; L.h_reward = {L.h_out.p + 2 * GA + n, n};
    L.d_policy = {L.d_out.p, GA}; L.d_logit = {L.d_out.p + GA, GA}; L.d_value = {L.d_out.p + 2 * GA, n}; L.d_reward = {L.d_out.p + 2 * GA + n, n};
    MZ_HIP(hipMemset(L.d_out.p, 0, L.d_out.n * sizeof(float)));
    if (desc_.type >= 1) { WALLOC(L.d_hidden, n * plan_.slab_slots * L.net->hiddenSize()); WALLOC(L.d_src_idx, n); WALLOC(L.d_dst_idx, n); WALLOC(L.d_action_ids, n); }
    if (rb > 0) {
        WALLOC(L.h_raw, n * rb); WALLOC(L.d_raw, n * rb);
        const int fb = games_[0].env->rawFrameBytes(), mb = plan_.raw_bytes - 8 * fb;
        if (fb > 0 && mb > 0 && mb <= 64) { WALLOC(L.h_new, n * fb); WALLOC(L.d_new, n * fb); WALLOC(L.h_meta, n * mb); WALLOC(L.d_meta, n * mb); WALLOC(L.d_raw2, n * rb); }
    }
    if (plan_.resident) {
        const GameEnv& e = *games_[0].env;
        const int* inv[8];
        const int* fwd[8];
        for (int r = 0; r < 8; ++r) { inv[r] = e.rot()->inv[r].data(); fwd[r] = e.rot()->fwd[r].data(); }
        rc = L.godev.init(device_, L.n, e.boardSize(), cfg_.env_go_komi, A_, n_ + 1, L.pool.v_.max_depth, L.stream, inv, fwd, e.zobristKeys(), e.deviceKind(), e.turnKey());
        if (rc) { return rc; }
    }
    if (plan_.sim_kernel) {
        WALLOC(L.h_rot, sims * n); WALLOC(L.d_rot, sims * n); WALLOC(L.h_noise, GA); WALLOC(L.d_noise, GA);
        if ((rc = L.makeSimEvents())) { return rc; }
    }
    if (plan_.dev_gumbel) { // the Gumbel state of every game (gumbel.h)
        const size_t k = n * (3 + kGumbelMaxSample);
        WALLOC(L.h_gum, k); WALLOC(L.d_gum, k);
        memset(L.h_gum.p, 0, k * sizeof(int));
        MZ_HIP(hipMemset(L.d_gum.p, 0, k * sizeof(int)));
    }
    if (plan_.sim_mz) { // root planes (bit-packed), legal mask and player of every game
        const size_t fw = plan_.sim_root_host ? 1 : games_[0].env->featureWords(), LW = (A_ + 63) / 64;
        WALLOC(L.h_rootfeat, n * fw); WALLOC(L.d_rootfeat, n * fw); WALLOC(L.h_rootlegal, n * LW); WALLOC(L.d_rootlegal, n * LW); WALLOC(L.h_rootturn, n); WALLOC(L.d_rootturn, n);
    }
    if (plan_.sim_mode.rounds) { // the network's counters of leaves evaluated ahead (adaptRounds)
        WALLOC(L.h_prestat, 512);
        memset(L.h_prestat.p, 0, 512 * sizeof(unsigned));
    }
#undef WALLOC
    return MZ_OK;
}

// A simulation that does not find its leaf evaluated ahead evaluates it itself, on ONE CU, while the round's launch — every other game of the pool — waits: one
// miss costs the move a whole evaluation's latency (150 us on BASELINE configs[4], where the second round of four misses in almost every move: the earlier
// simulations of the round move the value bounds, and the fourth visit of a root child is where a close arg-max flips).  A second expected leaf per simulation
// (mz_sim_round_alt) removes those misses but doubles the round's evaluations, so the rounds that do not fit the chip twice get it only while they keep needing it:
// per round, the share of recent moves in which one of its simulations missed (alt off) or took its second leaf (alt on), with hysteresis.  Which leaves are
// evaluated ahead never changes a record (sim.hip simPreProbe); the batched pipeline (sim_rounds.hip) evaluates the doubled round with two leaves per workgroup.
void Worker::adaptRounds()
{
    unsigned now[512] = {0};
    for (auto& L : lanes_) {
        if (!L->h_prestat.p) { return; }
        for (int i = 0; i < 512; ++i) { now[i] += L->h_prestat.p[i]; }
    }
    // (sim_pre_pair_kernel_mz: a partner workgroup stayed out — the GPU is shared.  Looked at whatever the second-leaf settings are: with mz_sim_round_alt=false every
    // small round goes to the pairs, and a shared GPU would pay the partner's bounded wait in every round of every move)
    if (now[129] != 0) { for (auto& L : lanes_) { L->net->pairTrouble(); if (L->net_b) { L->own_net->pairTrouble(); L->net_b->pairTrouble(); } } } // (a match: both sides' networks)
    if (!cfg_.mz_sim_round_alt || plan_.sim_mode.alt_base == 0) { return; }
    if (prestat_prev_.size() == 512) {
        const int cus = net0().cuCount();
        for (Round& rd : rounds_) {
            bool ev = false;
            for (int s = rd.s0; s < rd.s0 + rd.R && s < 126; ++s) { ev = ev || now[2 + s] != prestat_prev_[2 + s] || now[256 + s] != prestat_prev_[256 + s]; }
            rd.p_event = 0.875f * rd.p_event + (ev ? 0.125f : 0.0f);
            // what the second leaves cost the round (us on BASELINE configs[4]) against a miss's 150 us: a round that fits the chip twice gives up its pairs of
            // workgroups per leaf (~30; nothing where pairs are not available: always on), a larger one doubles its evaluations (~80, batched pipeline only)
            const bool small = 2 * G_ * rd.R <= cus;
            if (!small && !cfg_.mz_sim_round_batch) { rd.alt = false; continue; }
            const float cost = small ? (pairsUsable() ? 30.0f : 0.0f) : 80.0f;
            if (rd.p_event * 150.0f > 1.3f * cost || cost == 0.0f) { rd.alt = true; } else if (rd.p_event * 150.0f < 0.6f * cost) { rd.alt = false; }
        }
    }
    prestat_prev_.assign(now, now + 512);
}

int Worker::uploadRoots(Lane& L)
{
    const int g0 = L.g0;
    if (plan_.sim_mz) { // MuZero: what the initial inference and the root expansion need from the host engine
        const int fw = plan_.sim_root_host ? 1 : games_[0].env->featureWords(), LW = (A_ + 63) / 64;
        threads_->parallelFor(L.n, [this, &L, g0, fw, LW](int j) {
            Game& gm = games_[g0 + j];
            if (!plan_.sim_root_host) { gm.env->featureBits(0, L.h_rootfeat.p + size_t(j) * fw); }
            gm.env->legalMask(gm.legal.data());
            for (int w = 0; w < LW; ++w) { L.h_rootlegal.p[size_t(j) * LW + w] = 0; }
            for (int a = 0; a < A_; ++a) { if (gm.legal[a]) { L.h_rootlegal.p[size_t(j) * LW + (a >> 6)] |= 1ull << (a & 63); } }
            L.h_rootturn.p[j] = gm.env->turn();
        });
        MZ_HIP(hipMemcpyAsync(L.d_rootfeat.p, L.h_rootfeat.p, L.h_rootfeat.n * sizeof(uint32_t), hipMemcpyHostToDevice, L.stream));
        MZ_HIP(hipMemcpyAsync(L.d_rootlegal.p, L.h_rootlegal.p, L.h_rootlegal.n * sizeof(unsigned long long), hipMemcpyHostToDevice, L.stream));
        MZ_HIP(hipMemcpyAsync(L.d_rootturn.p, L.h_rootturn.p, L.h_rootturn.n * sizeof(int), hipMemcpyHostToDevice, L.stream));
        return MZ_OK;
    }
    threads_->parallelFor(L.n, [this, &L, g0](int j) { games_[g0 + j].env->exportDeviceRoot(L.godev.hostSnap(j)); });
    return L.godev.uploadRoots();
}

int Worker::createActors()
{
    // ref mode_handler.cpp:62 (main-thread seed) + actor_group.cpp:179-187 (createActors -> reset() draws the resign coin
    // from the MAIN thread's generator) + actor_group.cpp:66-70 (slave thread 0 seeds its own generator: seed + 0)
    const int seed = cfg_.program_auto_seed ? static_cast<int>(std::random_device()()) : cfg_.program_seed;
    main_rng_.seed(seed);
    games_.resize(G_);
    for (auto& g : games_) {
        // ref atari.cpp:87: observations kept for the OBS tag of the next record
        const size_t recent_obs = static_cast<size_t>(cfg_.zero_actor_intermediate_sequence_length == 0
                                                          ? 108000
                                                          : cfg_.zero_actor_intermediate_sequence_length + 8 + cfg_.learner_n_step_return + cfg_.learner_muzero_unrolling_step) + 1;
        g.env = createGameEnv(envOptions(cfg_, recent_obs));
        if (!g.env) { return MZ_ERR_ARG; }
        if (external_ && &g == &games_[0]) { int rx = extCheckDesc(*g.env); if (rx) { return rx; } }
        if (g.env->policySize() != A_ || g.env->featureSize() != feat_size_) {
            setError("network (A=%d, features=%d) does not fit env %s (A=%d, features=%d)", A_, feat_size_, g.env->name().c_str(),
                     g.env->policySize(), g.env->featureSize());
            return MZ_ERR_ARG;
        }
        g.leaf = g.env->clone();
        g.legal.assign(A_, 0);
        if (g.env->needsSeed()) {
            (void)main_rng_.randInt();                 // the reference env's constructor already resets once (atari.h:47-50)
            g.env->resetSeed(main_rng_.randInt());     // BaseActor::reset -> env_.reset() (atari.h:54)
        } else {
            g.env->reset();
        }
        g.action_info_history.clear();
        g.enable_resign = (main_rng_.randReal() < cfg_.zero_disable_resign_ratio ? false : true);
    }
    streams_ = std::max(1, cfg_.mz_rng_streams == 0 ? cfg_.zero_num_threads : cfg_.mz_rng_streams);
    rngs_.assign(streams_, Rng());
    for (int t = 0; t < streams_; ++t) { rngs_[t].seed(cfg_.program_auto_seed ? static_cast<int>(std::random_device()()) : cfg_.program_seed + t); }
    stream_noise_.assign(streams_, {});
    return MZ_OK;
}

int Worker::resetAllSearches(const uint8_t* mask) // mask: [G_], 0 = the game's tree stays (mz_think_reuse_tree)
{
    for (auto& L : lanes_) {
        std::vector<int> rp(L->n);
        for (int j = 0; j < L->n; ++j) { rp[j] = rootPlayerFor(games_[L->g0 + j]); }
        int rc = L->pool.resetSearch(mask ? mask + L->g0 : nullptr, rp.data());
        if (rc) { return rc; }
        if ((plan_.resident || plan_.sim_mz) && (rc = uploadRoots(*L))) { return rc; }
    }
    return MZ_OK;
}

void Worker::resetGame(Game& g, Rng& rng)
{
    if (g.env->needsSeed()) { g.env->resetSeed(rng.randInt()); } else { g.env->reset(); }
    g.action_info_history.clear();
    g.enable_resign = (rng.randReal() < cfg_.zero_disable_resign_ratio ? false : true);
}

// ------------------------------------------------------------------------------------------------
// candidates: ref zero_actor.cpp:215-245
void Worker::buildCandidates(int gi)
{
    Game& g = games_[gi];
    Lane& L = laneOf(gi);
    const int j = gi - L.g0; // index inside the lane
    const size_t off = size_t(j) * A_;
    int* ca = L.pool.h_cand_action_.p + off;
    float* cp = L.pool.h_cand_policy_.p + off;
    float* cl = L.pool.h_cand_logit_.p + off;
    const float* policy = L.h_policy.p + off;
    const float* logit = L.h_logit.p + off;
    Cand tmp[512];
    std::vector<Cand> big;
    Cand* c = tmp;
    if (A_ > 512) { big.resize(A_); c = big.data(); }
    int k = 0;
    float value = L.h_value.p[j], reward = 0.0f;
    int player;
    if (desc_.type == 0) {
        player = g.leaf_turn;
        reward = g.leaf_reward;
        if (g.leaf_terminal) {
            value = g.leaf_eval; // ref zero_actor.cpp:85: backup(path, env_transition.getEvalScore(), reward)
        } else {
            const int* fwd = g.env->rot()->fwd[g.rot].data();
            for (int a = 0; a < A_; ++a) {
                if (!g.legal[a]) { continue; }
                c[k++] = Cand{a, policy[fwd[a]], logit[fwd[a]]};
            }
        }
    } else {
        const int depth = g.path_len - 1; // depth of the leaf; its children are moved by the player to move there
        player = (g.env->numPlayers() == 2 && (depth & 1)) ? 3 - g.env->turn() : g.env->turn();
        reward = L.h_reward.p[j];
        if (desc_.type == 2) { // 601-bin heads: the kernels return the softmax expectation, the double-libm inverse stays here
            value = invertValueHost(value);
            reward = invertValueHost(reward);
        }
        for (int a = 0; a < A_; ++a) {
            if (depth == 0 && !g.legal[a]) { continue; } // legality is only known (and checked) at the root (zero_actor.cpp:238)
            c[k++] = Cand{a, policy[a], logit[a]};
        }
    }
    std::sort(c, c + k, [](const Cand& l, const Cand& r) { return l.policy > r.policy; }); // the reference's (unstable) std::sort
    for (int i = 0; i < k; ++i) { ca[i] = c[i].action; cp[i] = c[i].policy; cl[i] = c[i].logit; }
    L.pool.h_cand_count_.p[j] = k;
    L.pool.h_cand_player_.p[j] = player;
    L.pool.h_value_.p[j] = value;
    L.pool.h_reward_.p[j] = reward;
}

// leaf environment + features: ref zero_actor.cpp:51-72, 247-252
void Worker::buildLeaf(int gi)
{
    Game& g = games_[gi];
    Lane& L = laneOf(gi);
    const int j = gi - L.g0;
    const int len = L.pool.h_path_len_.p[j];
    g.path_len = len;
    float* feat = L.h_feat.p + size_t(j) * L.net->featSize();
    if (desc_.type == 0) {
        const int* acts = L.pool.h_path_action_.p + size_t(j) * L.pool.v_.max_depth;
        g.leaf->copyFrom(*g.env);
        int p = g.env->turn();
        for (int d = 1; d < len; ++d) {
            g.leaf->actUnchecked(acts[d], p);
            if (g.env->numPlayers() == 2) { p = 3 - p; }
        }
        g.leaf_terminal = g.leaf->isTerminal();
        g.leaf_turn = g.leaf->turn();
        g.leaf_reward = g.leaf->reward();
        if (g.leaf_terminal) { g.leaf_eval = g.leaf->evalScore(false); }
        else { g.leaf->legalMask(g.legal.data()); }
        if (plan_.feat_bits) { g.leaf->featureBits(g.rot, reinterpret_cast<uint32_t*>(L.h_feat.p) + size_t(j) * g.env->featureWords()); }
        else { g.leaf->features(g.rot, feat); }
    } else if (sims_done_ == 0) {
        if (plan_.raw_bytes > 0 && L.raw_incremental) {
            const int fb = g.env->rawFrameBytes(), mb = plan_.raw_bytes - 8 * fb;
            g.env->rawNewest(L.h_new.p + size_t(j) * fb, L.h_meta.p + size_t(j) * mb);
            g.raw_seen = g.env->rawSerial();
        } else if (plan_.raw_bytes > 0) {
            g.env->rawFeatures(L.h_raw.p + size_t(j) * plan_.raw_bytes);
            g.raw_seen = g.env->rawSerial();
        } else { g.env->features(0, feat); }
        g.env->legalMask(g.legal.data());
    }
}

// ------------------------------------------------------------------------------------------------
// host logic on root statistics
float Worker::normalizedMean(float reward, float mean, float count, int player, int g, float vl) const // ref mcts.cpp:40-53; vl: the node's virtual loss (batched think: thinkCycle)
{
    float value = reward + cfg_.actor_mcts_reward_discount * mean;
    if (cfg_.actor_mcts_value_rescale) {
        if (rr_bsize_[g] < 2) { return 1.0f; }
        const float lo = rr_lo_[g], hi = rr_hi_[g];
        value = (value - lo) / (hi - lo);
        value = ::fmin(static_cast<double>(1), ::fmax(static_cast<double>(-1), static_cast<double>(2 * value - 1)));
    }
    value = (player == flipping_player_ ? -value : value);
    value = (value * count - vl) / (count + vl);
    return value;
}

int Worker::selectChildByMaxCount(int g) const // ref mcts.cpp:91-104
{
    const size_t off = size_t(g) * A_;
    float max_count = 0.0f;
    int selected = -1;
    for (int i = 0; i < rr_nc_[g]; ++i) {
        if (rr_count_[off + i] <= max_count) { continue; }
        max_count = rr_count_[off + i];
        selected = i;
    }
    return selected;
}

int Worker::selectChildBySoftmaxCount(int g, float temperature, float value_threshold) // ref mcts.cpp:106-124
{
    const size_t off = size_t(g) * A_;
    const int child_player = games_[g].env->turn();
    int selected = -1;
    const int best = selectChildByMaxCount(g);
    const float best_mean = normalizedMean(rr_reward_[off + best], rr_mean_[off + best], rr_count_[off + best], child_player, g, vlOf(g, best));
    float sum = 0.0f;
    const float exponent = 1 / temperature;
    for (int i = 0; i < rr_nc_[g]; ++i) {
        // powf(x, 1.0f) == x bit for bit (tests/csrc/pow_one_check.cpp), and an unvisited child is skipped before its mean is looked at:
        // this loop runs over ~17 k children per move of BASELINE configs[1] between two launches
        const float count = exponent == 1.0f ? rr_count_[off + i] : std::pow(rr_count_[off + i], exponent);
        if (count == 0) { continue; }
        const float mean = normalizedMean(rr_reward_[off + i], rr_mean_[off + i], rr_count_[off + i], child_player, g, vlOf(g, i));
        if (mean < best_mean - value_threshold) { continue; }
        sum += count;
        float rand = rngOf(g).randReal(sum);
        if (selected == -1 || rand < count) { selected = i; }
    }
    return selected;
}

bool Worker::isResign(int g) const // ref mcts.cpp:84-89, zero_actor.h:40
{
    const Game& gm = games_[g];
    if (!gm.enable_resign) { return false; }
    const size_t off = size_t(g) * A_;
    // the root's own reward field is only ever written by the first backup of the search with the root-evaluation
    // reward, which is 0 for every environment this worker supports
    const float root_win_rate = normalizedMean(0.0f, rr_root_mean_[g], rr_root_count_[g], rootPlayerFor(gm), g, vlOf(g, -1));
    const int s = gm.selected;
    const float action_win_rate = normalizedMean(rr_reward_[off + s], rr_mean_[off + s], rr_count_[off + s], gm.env->turn(), g, vlOf(g, s));
    return (-root_win_rate < cfg_.actor_resign_threshold && action_win_rate < cfg_.actor_resign_threshold);
}

std::string Worker::searchDistributionString(int g) const // ref mcts.cpp:126-137
{
    const size_t off = size_t(g) * A_;
    std::ostringstream oss;
    bool first = true;
    for (int i = 0; i < rr_nc_[g]; ++i) {
        if (rr_count_[off + i] == 0) { continue; }
        oss << (first ? "" : ",") << rr_action_[off + i] << ":" << rr_count_[off + i];
        first = false;
    }
    return oss.str();
}

std::string Worker::gumbelPolicyString(int g, int child_player) const // ref gumbel_zero.cpp:9-58
{
    const size_t off = size_t(g) * A_;
    const int nc = rr_nc_[g];
    float pi_sum = 0.0f, q_sum = 0.0f;
    for (int i = 0; i < nc; ++i) {
        if (rr_count_[off + i] == 0) { continue; }
        float value = normalizedMean(rr_reward_[off + i], rr_mean_[off + i], rr_count_[off + i], child_player, g);
        pi_sum += rr_policy_[off + i];
        q_sum += rr_policy_[off + i] * value;
    }
    float value_pi = rr_root_value_[g];
    if (cfg_.actor_mcts_value_rescale) {
        if (rr_bsize_[g] < 2) {
            value_pi = 1.0f;
        } else {
            value_pi = (value_pi - rr_lo_[g]) / (rr_hi_[g] - rr_lo_[g]);
            value_pi = ::fmin(static_cast<double>(1), ::fmax(static_cast<double>(-1), static_cast<double>(2 * value_pi - 1)));
        }
    }
    value_pi = (child_player == flipping_player_ ? -value_pi : value_pi);
    float non_visited_node_value = 1.0 / (1 + cfg_.actor_num_simulation) * (value_pi + (cfg_.actor_num_simulation / pi_sum) * q_sum);
    std::unordered_map<int, float> new_logits; // its iteration order is part of the record format
    float max_logit = -std::numeric_limits<float>::max();
    float max_child_count = 0;
    for (int i = 0; i < nc; ++i) { max_child_count = ::fmax(static_cast<double>(max_child_count), static_cast<double>(rr_count_[off + i])); }
    for (int i = 0; i < nc; ++i) {
        float value = (rr_count_[off + i] == 0 ? non_visited_node_value
                                               : normalizedMean(rr_reward_[off + i], rr_mean_[off + i], rr_count_[off + i], child_player, g));
        float logit_without_noise = rr_logit_[off + i] - rr_noise_[off + i];
        float score = logit_without_noise + (cfg_.actor_gumbel_sigma_visit_c + max_child_count) * cfg_.actor_gumbel_sigma_scale_c * value;
        new_logits.insert({rr_action_[off + i], score});
        max_logit = ::fmax(static_cast<double>(max_logit), static_cast<double>(score));
    }
    std::ostringstream oss;
    for (auto& logit : new_logits) {
        logit.second = logit.second - max_logit;
        if (logit.second < -38) { continue; }
        oss << (oss.str().empty() ? "" : ",") << logit.first << ":" << ::exp(static_cast<double>(logit.second));
    }
    return oss.str();
}

void Worker::gumbelSortByScore(int g) // ref gumbel_zero.cpp:121-137
{
    const size_t off = size_t(g) * A_;
    const int child_player = games_[g].env->turn();
    float max_child_count = 0;
    for (int i = 0; i < rr_nc_[g]; ++i) { max_child_count = ::fmax(static_cast<double>(max_child_count), static_cast<double>(rr_count_[off + i])); }
    auto score = [&](int i) {
        float min_value = -std::numeric_limits<float>::max();
        float value = normalizedMean(rr_reward_[off + i], rr_mean_[off + i], rr_count_[off + i], child_player, g);
        float s = rr_logit_[off + i] + (cfg_.actor_gumbel_sigma_visit_c + max_child_count) * cfg_.actor_gumbel_sigma_scale_c * value;
        return (rr_count_[off + i] > 0 ? s : min_value);
    };
    std::sort(games_[g].candidates.begin(), games_[g].candidates.end(), [&](int l, int r) { return score(l) > score(r); });
}

void Worker::gumbelSequentialHalving(int g) // ref gumbel_zero.cpp:90-119
{
    Game& gm = games_[g];
    const size_t off = size_t(g) * A_;
    if (sim_post_ == 1) {
        gm.candidates.clear();
        for (int i = 0; i < rr_nc_[g]; ++i) { gm.candidates.push_back(i); }
        std::sort(gm.candidates.begin(), gm.candidates.end(), [&](int l, int r) { return rr_logit_[off + l] > rr_logit_[off + r]; });
        if (static_cast<int>(gm.candidates.size()) > cfg_.actor_gumbel_sample_size) { gm.candidates.resize(cfg_.actor_gumbel_sample_size); }
        gm.sample_size = cfg_.actor_gumbel_sample_size;
        gm.simulation_budget = std::max(1.0, std::floor(cfg_.actor_num_simulation / (std::log2(cfg_.actor_gumbel_sample_size) * gm.sample_size)));
    } else {
        bool all = true;
        for (int i : gm.candidates) {
            if (rr_count_[off + i] >= gm.simulation_budget) { continue; }
            all = false;
            break;
        }
        if (all) {
            int next_budget = std::floor(cfg_.actor_num_simulation / (std::log2(cfg_.actor_gumbel_sample_size) * gm.sample_size / 2));
            if (next_budget > 0 && gm.sample_size > 2) {
                gm.sample_size /= 2;
                gumbelSortByScore(g);
                if (static_cast<int>(gm.candidates.size()) > gm.sample_size) { gm.candidates.resize(gm.sample_size); }
                gm.simulation_budget = rr_count_[off + gm.candidates[0]] + next_budget;
            }
        }
    }
}

int Worker::decideAction(int g) // ref zero_actor.cpp:178-192, gumbel_zero.cpp:60-72
{
    if (cfg_.actor_use_gumbel && cfg_.actor_select_action_by_count) {
        gumbelSortByScore(g);
        return games_[g].candidates[0];
    }
    if (!cfg_.actor_use_gumbel && cfg_.actor_select_action_by_count) { return selectChildByMaxCount(g); }
    if (cfg_.actor_select_action_by_softmax_count) { return selectChildBySoftmaxCount(g, cfg_.actor_select_action_softmax_temperature); }
    return selectChildByMaxCount(g);
}

ActionInfo Worker::actionInfo(int g, int child_player) const // ref base_actor.cpp:59-66, zero_actor.h:50-51, zero_actor.cpp:121-126
{
    ActionInfo info;
    info.push_back({"P", cfg_.actor_use_gumbel ? gumbelPolicyString(g, child_player) : searchDistributionString(g)});
    info.push_back({"V", std::to_string(rr_root_mean_[g])});
    std::ostringstream oss;
    oss << games_[g].env->reward();
    info.push_back({"R", oss.str()});
    return info;
}

static const char kObsPlaceholder[] = "\x01OBS\x01";

std::string Worker::record(const Game& gm, const ActionInfo& extra, std::string* obs_raw) const // ref base_actor.cpp:39-57, base_env.h:207-233
{
    ActionInfo tags;
    auto addTag = [&](const std::string& k, const std::string& v) {
        for (auto& t : tags) { if (t.first == k) { t.second = v; return; } }
        tags.push_back({k, v});
    };
    addTag("GM", gm.env->name());
    addTag("RE", std::to_string(gm.env->evalScore(false)));
    if (!gm.env->hasObservations()) {
        addTag("OBS", ""); // compressString("") == "" (utils.h:37): board games keep no observations
    } else if (obs_raw) {
        obs_raw->clear();
        gm.env->appendObservations(obs_raw);
        addTag("OBS", kObsPlaceholder);
    } else { // ref base_env.h:216-220
        std::string raw, hex;
        gm.env->appendObservations(&raw);
        (void)compressToHex(reinterpret_cast<const uint8_t*>(raw.data()), raw.size(), &hex);
        addTag("OBS", hex);
    }
    for (auto& t : gm.env->loaderTags()) { addTag(t.first, t.second); }
    addTag("EV", cfg_.nn_file_name.substr(cfg_.nn_file_name.find_last_of('/') + 1));
    if (!gm.env->isTerminal()) { // unfinished game = resigned: the player to move loses (base_actor.cpp:49-54)
        std::ostringstream oss;
        oss << gm.env->evalScore(true);
        addTag("RE", oss.str());
    }
    for (auto& t : extra) { addTag(t.first, t.second); }
    std::ostringstream oss;
    oss << "(;";
    for (const auto& t : tags) { oss << t.first << "[" << escapeSGF(t.second) << "]"; }
    const auto& ids = gm.env->actionIds();
    const auto& pls = gm.env->actionPlayers();
    const std::vector<int>* lives = gm.env->livesHistory(); // ref atari.cpp:187-197: L[lives] on the action before which a life was lost
    int previous_lives = lives && !lives->empty() ? (*lives)[0] : 0;
    for (size_t i = 0; i < ids.size(); ++i) {
        oss << ";" << (pls[i] == 1 ? 'B' : 'W') << "[" << ids[i] << "]";
        bool lost = false;
        int now = previous_lives;
        if (lives && i < lives->size()) { now = (*lives)[i]; lost = now < previous_lives; previous_lives = now; }
        if (gm.action_info_history.size() > i) {
            for (const auto& info : gm.action_info_history[i]) {
                const bool is_l = lost && info.first == "L"; // VectorMap: an existing key keeps its place and takes the new value
                oss << info.first << "[" << escapeSGF(is_l ? std::to_string(now) : info.second) << "]";
                if (is_l) { lost = false; }
            }
        }
        if (lost) { oss << "L[" << now << "]"; }
    }
    oss << ")";
    return oss.str();
}

std::pair<int, int> Worker::trainingDataRange(const Game& gm) const // ref actor_group.cpp:52-64
{
    int game_length = static_cast<int>(gm.env->actionIds().size());
    int data_start = 0, data_end = game_length - 1;
    const int seq = cfg_.zero_actor_intermediate_sequence_length;
    if (seq > 0) {
        const int un = cfg_.learner_muzero_unrolling_step + cfg_.learner_n_step_return;
        const bool term = gm.env->isTerminal();
        data_end = std::max(0, (term ? data_end : data_end - un));
        data_start = std::max(0, (term ? data_end - data_end % seq : data_end + 1 - seq));
        if (term && (data_end % seq < un)) { data_start = std::max(0, data_start - seq); }
    }
    return {data_start, data_end};
}

void Worker::outputGame(Game& gm) // ref actor_group.cpp:24-50
{
    const int game_length = static_cast<int>(gm.env->actionIds().size());
    const std::pair<int, int> range = trainingDataRange(gm);
    const bool is_terminal = (cfg_.zero_actor_intermediate_sequence_length == 0 || gm.env->isTerminal());
    std::ostringstream oss;
    std::string obs_raw;
    ActionInfo tags = {{"DLEN", std::to_string(range.first) + "-" + std::to_string(range.second)}};
    if (match_) { tags.push_back({"PB", matchName(gm.m_first_side)}); tags.push_back({"PW", matchName(1 - gm.m_first_side)}); } // who had which colour
    oss << (match_ ? "Match " : "SelfPlay ") << (is_terminal ? "true" : "false") << " " << (range.second - range.first + 1) << " " << game_length << " "
        << gm.env->evalScore(!gm.env->isTerminal()) << " "
        << record(gm, tags, &obs_raw) << " "
        << "#";
    if (!is_terminal) {
        // (i < size: a resignation before the first move of an intermediate-sequence game has range 0-0 and an EMPTY history — the reference indexes it anyway)
        for (int i = range.first; i <= range.second && i < static_cast<int>(gm.action_info_history.size()); ++i) { gm.action_info_history[i].clear(); gm.action_info_history[i].shrink_to_fit(); }
    }
    auto line = std::make_unique<OutLine>();
    line->text = oss.str();
    const bool has_obs = gm.env->hasObservations();
    if (is_terminal) { if (tl_sink_) { ++tl_sink_->games; } else { ++stats_.games; } }
    if (tl_sink_) { tl_sink_->lines.push_back({std::move(line), std::move(obs_raw), has_obs}); }
    else { queueLine(std::move(line), std::move(obs_raw), has_obs); }
}

void Worker::queueLine(std::unique_ptr<OutLine> line, std::string&& obs_raw, bool has_obs)
{
    lines_.push_back(std::move(line));
    if (has_obs) {
        // (helpers: the host threads the configuration grants beyond the caller's, at least one — they sleep when there is nothing to compress)
        if (!obs_) { obs_ = std::make_unique<ObsCompressor>(std::max(1, hostThreads() - 1)); }
        obs_->submit(lines_.back().get(), std::move(obs_raw), kObsPlaceholder, sizeof(kObsPlaceholder) - 1);
    }
}

void Worker::handleSearchDone(int g) // ref actor_group.cpp:116-134 + base_actor.cpp:22-30
{
    Game& gm = games_[g];
    const size_t off = size_t(g) * A_;
    const bool resign = isResign(g);
    if (cfg_.mz_manual_step) { // the caller plays: keep what ZeroActor::handleSearchDone leaves behind (zero_actor.cpp:128-176)
        Held& h = held_[g];
        h.action = rr_action_[off + gm.selected];
        h.player = gm.env->turn();
        h.resign = resign;
        h.info = rr_root_count_[g] > 0 ? actionInfo(g, h.player) : ActionInfo(); // ZeroActor::getActionInfo (zero_actor.cpp:114-119)
        return;
    }
    bool acted = false;
    int mover = 0;
    if (!resign) {
        const int action = rr_action_[off + gm.selected];
        mover = gm.env->turn(); // == the player of every root child
        if (gm.env->act(action, mover)) {
            gm.action_info_history.resize(gm.env->actionIds().size());
            acted = true;
        }
    }
    if (tl_sink_) { ++tl_sink_->moves; } else { ++stats_.moves; }
    const bool is_endgame = (resign || gm.env->isTerminal());
    const int game_length = static_cast<int>(gm.env->actionIds().size());
    const int seq = cfg_.zero_actor_intermediate_sequence_length;
    const bool intermediate = !is_endgame && seq > 0 && game_length >= seq &&
                              (game_length - cfg_.learner_n_step_return - cfg_.learner_muzero_unrolling_step) % seq == 0;
    if (acted) {
        // the P/V/R strings of this move (no RNG involved) are only needed when the game is printed: for every other game they are
        // built after the next launch has been queued, off the critical path (the root statistics stay valid until the next root read)
        if (plan_.defer_info && !is_endgame && !intermediate) { (tl_sink_ ? tl_sink_->deferred : deferred_).push_back({g, mover, gm.action_info_history.size() - 1}); }
        else { gm.action_info_history.back() = actionInfo(g, mover); }
    }
    if (match_) { // what matchAfterMoves tallies, taken before the slot's next game starts
        gm.m_acted = acted;
        gm.m_ended = is_endgame;
        gm.m_resigned = is_endgame && resign;
        if (is_endgame) { gm.m_score = gm.env->evalScore(!gm.env->isTerminal()); }
    }
    if (is_endgame) {
        if (!match_ || gm.m_serial >= 0) { outputGame(gm); } // (a filler game of a match is never printed)
        resetGame(gm, rngOf(g));
    } else if (intermediate) {
        outputGame(gm);
    }
}

void Worker::flushDeferred()
{
    if (deferred_.empty()) { return; }
    threads_->parallelFor(static_cast<int>(deferred_.size()), [this](int k) {
        const DeferredInfo& d = deferred_[k];
        games_[d.g].action_info_history[d.index] = actionInfo(d.g, d.mover);
    });
    deferred_.clear();
}

thread_local Worker::StreamSink* Worker::tl_sink_ = nullptr;

void Worker::drawRootNoise(int g, std::vector<float>& noise) // ref zero_actor.cpp:194-213
{
    const size_t off = size_t(g) * A_;
    const int k = rr_nc_[g];
    if (cfg_.actor_use_dirichlet_noise) {
        const float epsilon = cfg_.actor_dirichlet_noise_epsilon;
        rngOf(g).dirichlet(cfg_.actor_dirichlet_noise_alpha, k, noise);
        for (int i = 0; i < k; ++i) {
            rr_noise_[off + i] = noise[i];
            rr_policy_[off + i] = (1 - epsilon) * rr_policy_[off + i] + epsilon * noise[i];
        }
    } else {
        rngOf(g).gumbel(k, noise);
        for (int i = 0; i < k; ++i) {
            rr_noise_[off + i] = noise[i];
            rr_logit_[off + i] = rr_logit_[off + i] + noise[i];
        }
    }
    memcpy(noise_policy_.data() + off, rr_policy_.data() + off, k * sizeof(float));
    memcpy(noise_logit_.data() + off, rr_logit_.data() + off, k * sizeof(float));
    memcpy(noise_noise_.data() + off, rr_noise_.data() + off, k * sizeof(float));
}

// the per-move host logic of one game, in the reference's order: [root noise][move decision + Gumbel bookkeeping + act / record / reset][rotation]
void Worker::serialGame(int g, bool want_noise, bool done, bool az, std::vector<float>& noise)
{
    Game& gm = games_[g];
    if (want_noise) { drawRootNoise(g, noise); }
    if (done) { gm.selected = decideAction(g); }                  // zero_actor.cpp:96 handleSearchDone()
    if (cfg_.actor_use_gumbel) { gumbelSequentialHalving(g); }     // zero_actor.cpp:97
    if (done) { handleSearchDone(g); }                             // actor_group.cpp:92
    if (az && !(done && cfg_.mz_manual_step)) { // beforeNNEvaluation: the rotation draw (zero_actor.cpp:56)
        gm.rot = cfg_.actor_use_random_rotation_features ? rngOf(g).randInt() % 8 : 0;
    }
}

// One stream: strictly serial, in actor index order (the deterministic contract).  Several streams (mz_rng_streams): every stream's block of games in index
// order on one thread of the pool, the blocks side by side; what they produce for the pool (finished records, counters, deferred record strings) is merged in
// stream order, which is game order — the lines leave exactly as the serial loop would have queued them.
void Worker::serialSection(Lane& L, bool want_noise, bool done, bool az)
{
    const int g0 = L.g0, g1 = L.g0 + L.n;
    if (streams_ == 1) {
        std::vector<float>& noise = stream_noise_[0];
        for (int g = g0; g < g1; ++g) { serialGame(g, want_noise, done, az, noise); }
        return;
    }
    sinks_.resize(streams_);
    threads_->parallelFor(streams_, [this, g0, g1, want_noise, done, az](int t) {
        const int gs = std::max(g0, static_cast<int>((static_cast<long long>(t) * G_ + streams_ - 1) / streams_));
        const int ge = std::min(g1, static_cast<int>((static_cast<long long>(t + 1) * G_ + streams_ - 1) / streams_));
        if (gs >= ge) { return; }
        tl_sink_ = &sinks_[t];
        for (int g = gs; g < ge; ++g) { serialGame(g, want_noise, done, az, stream_noise_[t]); }
        tl_sink_ = nullptr;
    });
    for (StreamSink& s : sinks_) {
        stats_.moves += s.moves; stats_.games += s.games;
        s.moves = s.games = 0;
        deferred_.insert(deferred_.end(), s.deferred.begin(), s.deferred.end());
        s.deferred.clear();
        for (auto& l : s.lines) { queueLine(std::move(l.line), std::move(l.obs_raw), l.has_obs); }
        s.lines.clear();
    }
}

// ------------------------------------------------------------------------------------------------
// phase 1 of a lane: consume the network outputs of the previous cycle (expand + backup), run the RNG-ordered serial
// section for the lane's games, then launch the selection of the next simulation (asynchronously).
int Worker::phase1(Lane& L, bool root_expansion, bool done, bool launch_select)
{
    const bool az = desc_.type == 0;
    const int g0 = L.g0, g1 = L.g0 + L.n;
    double t0 = nowMs();
    if (pending_) {
        double t1 = t0, te = t0;
        int rc = MZ_OK;
        if (!plan_.resident && (!plan_.sim_mz || root_host_pending_)) { // resident / simulation kernel: candidates + expand + backup already ran on the device
            // (root_host_pending_ is cleared by the caller when EVERY lane has had its turn: cleared here, the lanes behind the first kept unexpanded roots)
            if (cfg_.mz_signal_wait) { int rcw = L.pool.waitSignal(L.signal_seq); if (rcw) { return rcw; } }
            else { MZ_HIP(hipStreamSynchronize(L.stream)); } // network outputs of this lane
            t1 = nowMs();
            stats_.ms_forward += t1 - t0;
            trace_.add(0, t1 - t0);
            threads_->parallelFor(L.n, [this, g0](int j) { buildCandidates(g0 + j); });
            const double tc = nowMs();
            trace_.add(1, tc - t1);
            rc = L.pool.expandBackupStaged(az ? -1 : sim_pre_);
            if (rc) { return rc; }
            te = nowMs();
            trace_.add(2, te - tc);
        }
        const bool want_noise = root_expansion && (cfg_.actor_use_dirichlet_noise || cfg_.actor_use_gumbel_noise);
        if (done || cfg_.actor_use_gumbel || want_noise) {
            // root statistics for the per-move host logic (sync point; also surfaces pool capacity errors)
            const size_t o = size_t(g0) * A_;
            rc = L.pool.rootRead(rr_nc_.data() + g0, rr_action_.data() + o, rr_count_.data() + o, rr_mean_.data() + o, rr_policy_.data() + o,
                                 rr_logit_.data() + o, rr_noise_.data() + o, rr_value_.data() + o, rr_reward_.data() + o, rr_root_count_.data() + g0,
                                 rr_root_mean_.data() + g0, rr_root_value_.data() + g0, rr_lo_.data() + g0, rr_hi_.data() + g0, rr_bsize_.data() + g0, L.rr_ahead);
            L.rr_ahead = false;
            if (rc) { return rc; }
            if ((rc = L.pool.checkError())) { return rc; }
        }
        const double t2 = nowMs();
        stats_.ms_expand += t2 - t1;
        trace_.add(3, t2 - te);
        // ---- the RNG-ordered section: actor index order within every RNG stream ----
        serialSection(L, want_noise, done, az);
        if (match_ && done) { // the move boundary of a match: the tally, the games that start, and the side that searches the lane in the next step
            matchAfterMoves(L);
            if ((rc = matchBeginStep(L, match_t_ + 1))) { return rc; }
        }
        const double ts = nowMs();
        trace_.add(4, ts - t2);
        if (want_noise) {
            const size_t o = size_t(g0) * A_;
            if ((rc = L.pool.rootSetNoise(noise_mask_.data() + g0, noise_policy_.data() + o, noise_logit_.data() + o, noise_noise_.data() + o))) { return rc; }
            trace_.add(11, nowMs() - ts);
        }
        if (done && !cfg_.mz_manual_step) {
            std::vector<int> rp(L.n);
            for (int j = 0; j < L.n; ++j) { rp[j] = rootPlayerFor(games_[g0 + j]); }
            const double tr0 = nowMs();
            if ((rc = L.pool.resetSearch(nullptr, rp.data()))) { return rc; }
            const double tr1 = nowMs();
            trace_.add(12, tr1 - tr0);
            if ((plan_.resident || plan_.sim_mz) && (rc = uploadRoots(L))) { return rc; }
            trace_.add(13, nowMs() - tr1);
        }
        if (done && cfg_.mz_manual_step) { return MZ_OK; } // no next selection: the caller acts and resets the search first
        t0 = nowMs();
        stats_.ms_move += t0 - t2;
        trace_.add(5, t0 - ts);
    } else {
        if (match_) { int rcm = matchBeginStep(L, match_t_); if (rcm) { return rcm; } }
        for (int g = g0; g < g1; ++g) {
            if (az) { games_[g].rot = cfg_.actor_use_random_rotation_features ? rngOf(g).randInt() % 8 : 0; }
        }
    }
    // ---- selection of the next simulation ----
    const int next_sim = pending_ ? (done ? 0 : sim_post_) : 0;
    const int* d_start = nullptr;
    if (cfg_.actor_use_gumbel && next_sim >= 1) { // ref gumbel_zero.cpp:74-88
        for (int g = g0; g < g1; ++g) {
            Game& gm = games_[g];
            const size_t off = size_t(g) * A_;
            std::sort(gm.candidates.begin(), gm.candidates.end(), [&](int l, int r) {
                return (rr_count_[off + l] < rr_count_[off + r] || (rr_count_[off + l] == rr_count_[off + r] && rr_logit_[off + l] > rr_logit_[off + r]));
            });
            L.pool.h_start_.p[g - g0] = 1 + gm.candidates[0]; // the root's children are nodes 1..k
        }
        MZ_HIP(hipMemcpyAsync(L.pool.d_start_.p, L.pool.h_start_.p, L.n * sizeof(int), hipMemcpyHostToDevice, L.stream));
        d_start = L.pool.d_start_.p;
    }
    if (!launch_select) { return MZ_OK; } // per-game simulation kernel: selection is part of the launch (runCyclesSim)
    if (plan_.resident) { for (int g = g0; g < g1; ++g) { rotPackSet(L.rot, g - g0, games_[g].rot); } }
    int rc = L.pool.selectAsync(d_start);
    if (rc) { return rc; }
    if (plan_.resident) {
        const double tz = nowMs();
        stats_.ms_select += tz - t0;
        return MZ_OK;
    }
    if (!(cfg_.mz_zero_copy & 2)) {
        // one D2H: [path_len n] (+ [path_action n*max_depth] for AlphaZero, whose leaves need the moves for the replay)
        MZ_HIP(hipMemcpyAsync(L.pool.h_path_arena_.p, L.pool.d_path_arena_.p,
                              (size_t(L.n) + (az ? size_t(L.n) * L.pool.v_.max_depth : 0)) * sizeof(uint32_t), hipMemcpyDeviceToHost, L.stream));
    } // else: select_kernel already wrote path_len / path_action into the pinned mirrors
    if (cfg_.mz_signal_wait) { int rcs = L.pool.signalAsync(++L.signal_seq); if (rcs) { return rcs; } }
    const double tz = nowMs();
    stats_.ms_select += tz - t0;
    trace_.add(6, tz - t0);
    return MZ_OK;
}

// phase 2 of a lane: leaf positions + feature planes on the host, then the network (asynchronously).
// device-resident cycle: leaf position + planes + legal mask, network, candidate lists, expand + backup — all queued, no host hop
int Worker::phase2Resident(Lane& L)
{
    const double t0 = nowMs();
    const int slot = sims_done_; // position slot of this simulation's leaf (slot 0 = the root)
    int rc;
    if ((rc = L.godev.leafAsync(L.pool.v_, L.rot, slot))) { return rc; }
    if (ext_) {
        // the hand-over: planes into the caller's tensor, wait, the caller's code (it returns with its outputs complete), its outputs into the lane's
        if ((rc = ext_->exportAsync(L.godev.v_.feat))) { return rc; }
        MZ_HIP(hipStreamSynchronize(L.stream));
        const int frc = ext_ev_.forward(ext_ev_.user, L.n);
        if (frc != 0) { // nothing of this cycle has reached a tree: the selection and the leaf position only wrote scratch of their own
            char text[160];
            snprintf(text, sizeof(text), "external evaluator: forward returned %d; the cycle was abandoned and the worker runs no further cycles", frc);
            ext_failed_ = text;
            setError("%s", text);
            return MZ_ERR_STATE;
        }
        MZ_HIP(hipSetDevice(device_)); // (the caller's code may have chosen another device for this thread)
        if ((rc = ext_->importAsync(L.d_policy.p, L.d_logit.p, L.d_value.p))) { return rc; }
    } else if ((rc = L.net->forwardAZ(reinterpret_cast<const float*>(L.godev.v_.feat), L.n, L.d_policy.p, L.d_logit.p, L.d_value.p, true))) { return rc; }
    if ((rc = L.godev.candAsync(L.pool, L.d_policy.p, L.d_logit.p, L.d_value.p, L.rot))) { return rc; }
    if ((rc = L.pool.expandBackupAsync(slot, false))) { return rc; }
    // bound the host's run-ahead (kernel-argument ring, launch queue): a completion word every 32 cycles, wait for the one before
    if (++L.cycles_since_signal >= 32) {
        L.cycles_since_signal = 0;
        if (L.signal_seq > 0 && (rc = L.pool.waitSignal(L.signal_seq))) { return rc; }
        if ((rc = L.pool.signalAsync(++L.signal_seq))) { return rc; }
    }
    stats_.ms_forward += nowMs() - t0;
    return MZ_OK;
}

int Worker::phase2(Lane& L)
{
    if (plan_.resident) { return phase2Resident(L); }
    const bool az = desc_.type == 0;
    const int g0 = L.g0;
    const double t0 = nowMs();
    if (cfg_.mz_signal_wait) { int rcw = L.pool.waitSignal(L.signal_seq); if (rcw) { return rcw; } }
    else { MZ_HIP(hipStreamSynchronize(L.stream)); } // paths of this lane
    const double t1 = nowMs();
    stats_.ms_select += t1 - t0;
    trace_.add(7, t1 - t0);
    if (plan_.raw_bytes > 0 && sims_done_ == 0) { // root observations: newest screen only when every game's previous block is on the device
        bool inc = L.raw_have && L.d_raw2.p != nullptr;
        for (int j = 0; inc && j < L.n; ++j) {
            const Game& gm = games_[g0 + j];
            inc = gm.env->rawSerial() == gm.raw_seen + 1 || gm.env->rawValidCount() == 1;
        }
        L.raw_incremental = inc;
    }
    threads_->parallelFor(L.n, [this, g0](int j) { buildLeaf(g0 + j); });
    const double t2 = nowMs();
    stats_.ms_env += t2 - t1;
    trace_.add(8, t2 - t1);
    int rc;
    if (az) {
        const size_t fbytes = plan_.feat_bits ? size_t(L.n) * games_[0].env->featureWords() * sizeof(uint32_t) : size_t(L.n) * L.net->featSize() * sizeof(float);
        // zero-copy: the tower kernel stages its LDS tile straight from pinned host memory / the heads kernel writes the outputs there
        const bool zin = cfg_.mz_zero_copy & 1, zout = cfg_.mz_zero_copy & 2;
        if (!zin) { MZ_HIP(hipMemcpyAsync(L.d_feat.p, L.h_feat.p, fbytes, hipMemcpyHostToDevice, L.stream)); }
        if ((rc = L.net->forwardAZ(zin ? L.h_feat.p : L.d_feat.p, L.n, zout ? L.h_policy.p : L.d_policy.p, zout ? L.h_logit.p : L.d_logit.p,
                                  zout ? L.h_value.p : L.d_value.p, plan_.feat_bits))) {
            return rc;
        }
        if (zout) {
            if (cfg_.mz_signal_wait) { if ((rc = L.pool.signalAsync(++L.signal_seq))) { return rc; } }
            const double t3z = nowMs();
            stats_.ms_forward += t3z - t2;
            trace_.add(9, t3z - t2);
            return MZ_OK;
        }
    } else if (sims_done_ == 0) {
        if (plan_.raw_bytes > 0 && L.raw_incremental) {
            const int fb = games_[g0].env->rawFrameBytes(), mb = plan_.raw_bytes - 8 * fb;
            uint8_t* prev = L.raw_cur == 0 ? L.d_raw.p : L.d_raw2.p;
            uint8_t* cur = L.raw_cur == 0 ? L.d_raw2.p : L.d_raw.p;
            MZ_HIP(hipMemcpyAsync(L.d_new.p, L.h_new.p, size_t(L.n) * fb, hipMemcpyHostToDevice, L.stream));
            MZ_HIP(hipMemcpyAsync(L.d_meta.p, L.h_meta.p, size_t(L.n) * mb, hipMemcpyHostToDevice, L.stream));
            if ((rc = L.net->shiftExpandAtariFeatures(prev, L.d_new.p, L.d_meta.p, cur, plan_.raw_bytes, L.n, L.d_feat.p))) { return rc; }
            L.raw_cur ^= 1;
        } else if (plan_.raw_bytes > 0) {
            uint8_t* cur = L.raw_cur == 0 ? L.d_raw.p : L.d_raw2.p;
            MZ_HIP(hipMemcpyAsync(cur, L.h_raw.p, size_t(L.n) * plan_.raw_bytes, hipMemcpyHostToDevice, L.stream));
            if ((rc = L.net->expandAtariFeatures(cur, plan_.raw_bytes, L.n, L.d_feat.p))) { return rc; }
            L.raw_have = true;
        } else {
            MZ_HIP(hipMemcpyAsync(L.d_feat.p, L.h_feat.p, size_t(L.n) * L.net->featSize() * sizeof(float), hipMemcpyHostToDevice, L.stream));
        }
        if ((rc = L.pool.hiddenIndexAsync(plan_.slab_slots, 0, L.d_src_idx.p, L.d_dst_idx.p, L.d_action_ids.p))) { return rc; }
        if ((rc = L.net->initial(L.d_feat.p, L.n, L.d_policy.p, L.d_logit.p, L.d_value.p, L.d_hidden.p, L.d_dst_idx.p))) { return rc; }
        MZ_HIP(hipMemsetAsync(L.d_reward.p, 0, L.n * sizeof(float), L.stream));
    } else {
        // device-resident MuZero step: parent hidden state gathered from the slab, action plane synthesised on device
        if ((rc = L.pool.hiddenIndexAsync(plan_.slab_slots, sims_done_, L.d_src_idx.p, L.d_dst_idx.p, L.d_action_ids.p))) { return rc; }
        if ((rc = L.net->recurrent(L.d_hidden.p, L.d_src_idx.p, nullptr, L.d_action_ids.p, L.n, L.d_policy.p, L.d_logit.p, L.d_value.p, L.d_reward.p,
                                  L.d_hidden.p, L.d_dst_idx.p))) {
            return rc;
        }
    }
    MZ_HIP(hipMemcpyAsync(L.h_out.p, L.d_out.p, L.h_out.n * sizeof(float), hipMemcpyDeviceToHost, L.stream));
    if (cfg_.mz_signal_wait) { if ((rc = L.pool.signalAsync(++L.signal_seq))) { return rc; } }
    const double t3 = nowMs();
    stats_.ms_forward += t3 - t2;
    trace_.add(9, t3 - t2);
    return MZ_OK;
}

int Worker::cycle()
{
    const double t0 = nowMs();
    MZ_HIP(hipSetDevice(device_));
    sim_pre_ = sims_done_;
    sim_post_ = sims_done_ + 1;
    const bool root_expansion = pending_ && (sim_post_ == 1), done = pending_ && (sim_post_ == n_ + 1);
    for (auto& L : lanes_) {
        int rc = phase1(*L, root_expansion, done);
        if (rc) { return rc; }
    }
    root_host_pending_ = false;
    if (done && cfg_.mz_manual_step) { search_done_ = true; stop_now_ = true; pending_ = false; sims_done_ = 0; return MZ_OK; }
    if (match_ && done) {
        ++match_t_;
        if (matchOver()) { // the N-th counted game has finished: what the boundary queued (search reset, roots, a selection) ends, and no further cycle runs
            match_done_ = true; stop_now_ = true; pending_ = false; sims_done_ = 0;
            for (auto& L : lanes_) {
                MZ_HIP(hipStreamSynchronize(L->stream));
                int rc = L->pool.checkError();
                if (rc) { return rc; }
            }
            return MZ_OK;
        }
    }
    if (pending_) { sims_done_ = done ? 0 : sim_post_; }
    for (auto& L : lanes_) {
        int rc = phase2(*L);
        if (rc) { return rc; }
    }
    pending_ = true;
    ++stats_.cycles;
    stats_.leaf_evals += G_;
    stats_.ms_total += nowMs() - t0;
    return MZ_OK;
}

// Gumbel state of the lane's games between host (Game::candidates / sample_size / simulation_budget) and device (gumbel.h layout)
int Worker::syncGumbel(Lane& L, bool to_device)
{
    const int stride = 3 + kGumbelMaxSample;
    if (to_device) {
        for (int j = 0; j < L.n; ++j) {
            const Game& gm = games_[L.g0 + j];
            int* st = L.h_gum.p + size_t(j) * stride;
            st[0] = static_cast<int>(gm.candidates.size());
            st[1] = gm.sample_size;
            st[2] = gm.simulation_budget;
            for (size_t i = 0; i < gm.candidates.size() && i < size_t(kGumbelMaxSample); ++i) { st[3 + i] = gm.candidates[i]; }
        }
        MZ_HIP(hipMemcpyAsync(L.d_gum.p, L.h_gum.p, L.h_gum.n * sizeof(int), hipMemcpyHostToDevice, L.stream));
        return MZ_OK;
    }
    MZ_HIP(hipMemcpyAsync(L.h_gum.p, L.d_gum.p, L.h_gum.n * sizeof(int), hipMemcpyDeviceToHost, L.stream));
    MZ_HIP(hipStreamSynchronize(L.stream));
    for (int j = 0; j < L.n; ++j) {
        Game& gm = games_[L.g0 + j];
        const int* st = L.h_gum.p + size_t(j) * stride;
        gm.candidates.assign(st + 3, st + 3 + std::max(0, std::min(st[0], kGumbelMaxSample)));
        gm.sample_size = st[1];
        gm.simulation_budget = st[2];
    }
    return MZ_OK;
}

// The RNG draws of the cycles [b0, b1) that join a launch: row b of the lanes' rotation tables (AlphaZero: one draw per game and cycle, zero_actor.cpp:56) and — cycle
// `noise_row` — the root noise of every game (its length is the number of legal moves, which the host engine knows; zero_actor.cpp:194-213).  Per stream the
// order is the reference's: cycle-major, actor-minor, [noise][rotation] per actor.  One stream (mz_rng_streams = 1, the deterministic contract): the calling
// thread; T streams: each is a contiguous block of games with its own generator, so the blocks are drawn side by side on the pool's threads (the 20 k gamma
// draws of 256 roots: 0.9 ms on one thread).  (Its own function: the hot loop of a 400-simulation move — 102 400 rotation draws per move on BASELINE
// configs[1] — must not depend on the inlining decisions inside runCyclesSim, which cost 1.4 ms per move once.)
__attribute__((noinline, aligned(64))) void Worker::drawStream(int t, int b0, int b1, int noise_row)
{
    const bool az = desc_.type == 0, rotate = cfg_.actor_use_random_rotation_features;
    // the games of stream t: [gs, ge) (streamOf is monotone)
    int gs = 0, ge = G_;
    if (streams_ > 1) {
        gs = static_cast<int>((static_cast<long long>(t) * G_ + streams_ - 1) / streams_);
        ge = static_cast<int>((static_cast<long long>(t + 1) * G_ + streams_ - 1) / streams_);
    }
    if (gs >= ge) { return; }
    Rng& rng = rngs_[t];
    std::vector<float>& scratch = stream_noise_[t];
    for (int b = b0; b < b1; ++b) {
        const bool noise_cycle = b == noise_row;
        if (!noise_cycle && !az) { continue; } // MuZero draws nothing in a plain cycle
        for (auto& L : lanes_) {
            const int j0 = std::max(gs, L->g0) - L->g0, j1 = std::min(ge, L->g0 + L->n) - L->g0;
            if (j0 >= j1) { continue; }
            uint8_t* rot_row = L->h_rot.p + size_t(b) * L->n;
            if (!noise_cycle) { // a plain cycle only fills its row of the rotation table (Game::rot is drawn again by the next phase1 before anybody reads it)
                for (int j = j0; j < j1; ++j) { rot_row[j] = rotate ? static_cast<uint8_t>(rng.randInt() % 8) : 0; }
                continue;
            }
            for (int j = j0; j < j1; ++j) {
                Game& gm = games_[L->g0 + j];
                gm.env->legalMask(gm.legal.data());
                int k = 0;
                for (int a = 0; a < A_; ++a) { k += gm.legal[a] != 0; }
                if (cfg_.actor_use_dirichlet_noise) { rng.dirichlet(cfg_.actor_dirichlet_noise_alpha, k, scratch); }
                else { rng.gumbel(k, scratch); }
                memcpy(L->h_noise.p + size_t(j) * A_, scratch.data(), size_t(k) * sizeof(float));
                if (az) { // AlphaZero: the only draw of a plain cycle (zero_actor.cpp:56); MuZero draws nothing
                    gm.rot = rotate ? rng.randInt() % 8 : 0;
                    rot_row[j] = static_cast<uint8_t>(gm.rot);
                }
            }
        }
    }
}

void Worker::drawCycles(int b0, int b1, int noise_row)
{
    if (b0 >= b1) { return; }
    if (streams_ == 1) { drawStream(0, b0, b1, noise_row); return; }
    threads_->parallelFor(streams_, [this, b0, b1, noise_row](int t) { drawStream(t, b0, b1, noise_row); });
}

// Device-resident cycles in batches: the host part of a cycle (per-move logic in RNG order, rotation draws) runs exactly as in
// cycle(); every following cycle that needs nothing from the host but its rotation draws joins the same launch of the per-game
// simulation kernel.  A 400-simulation move is two launches: the root expansion, then (after the root noise) the other 400.
int Worker::runCyclesSim(int n)
{
    MZ_HIP(hipSetDevice(device_));
    const bool noise_cfg = cfg_.actor_use_dirichlet_noise || cfg_.actor_use_gumbel_noise;
    int i = 0;
    while (i < n) {
        const double t0 = nowMs();
        sim_pre_ = sims_done_;
        sim_post_ = sims_done_ + 1;
        const bool root_expansion = pending_ && (sim_post_ == 1), done = pending_ && (sim_post_ == n_ + 1);
        const bool host_gumbel = plan_.dev_gumbel && pending_; // the host runs this cycle's Gumbel step itself: state down, step, state up
        // muzero_atari: the root's 96x96 representation is not part of the kernel; simulation 0 of a move runs as one lock-step cycle
        // (select, host planes, stand-alone kernels); its outputs are expanded on the device when simulations follow in this call (below), otherwise by
        // the next phase1 on the host; the other n simulations are one launch
        const bool root_cycle = plan_.sim_root_host && (!pending_ || done);
        for (auto& L : lanes_) {
            int rc = MZ_OK;
            if (host_gumbel && (rc = syncGumbel(*L, false))) { return rc; }
            if ((rc = phase1(*L, root_expansion, done, root_cycle))) { return rc; }
            if (host_gumbel && (rc = syncGumbel(*L, true))) { return rc; }
            for (int j = 0; j < L->n; ++j) { L->h_rot.p[j] = static_cast<uint8_t>(games_[L->g0 + j].rot); }
        }
        root_host_pending_ = false;
        if (done && cfg_.mz_manual_step) { search_done_ = true; pending_ = false; sims_done_ = 0; stats_.ms_total += nowMs() - t0; return i; }
        if (match_ && done) {
            ++match_t_;
            if (matchOver()) { // the N-th counted game has finished: what the boundary queued (search reset, roots) ends, and no further cycle runs
                match_done_ = true; pending_ = false; sims_done_ = 0;
                for (auto& L : lanes_) {
                    MZ_HIP(hipStreamSynchronize(L->stream));
                    int rc = L->pool.checkError();
                    if (rc) { return rc; }
                }
                stats_.ms_total += nowMs() - t0;
                return i;
            }
        }
        if (pending_) { sims_done_ = done ? 0 : sim_post_; }
        int sim0 = sims_done_;
        bool root_on_device = false;
        if (root_cycle) {
            for (auto& L : lanes_) {
                int rc = phase2(*L);
                if (rc) { return rc; }
            }
            { const double tf = nowMs(); flushDeferred(); trace_.add(14, nowMs() - tf); }
            pending_ = true;
            stats_.cycles += 1;
            stats_.leaf_evals += uint64_t(G_);
            i += 1;
            // mz_sim_split: when simulations follow in this call, the root is expanded on the device from the stand-alone kernels' outputs (simulation 0 of
            // the one-workgroup kernel with a given root) and the launch of simulations 1..n follows on the stream without a host round trip; the Gumbel /
            // Dirichlet noise of the root children is drawn meanwhile (its values only depend on the RNG stream and the number of legal actions).
            root_on_device = cfg_.mz_sim_split && i < n && n_ >= 1;
            if (!root_on_device) {
                root_host_pending_ = true; // the next phase1 expands the root on the host
                stats_.ms_total += nowMs() - t0;
                trace_.add(16, nowMs() - t0);
                continue;
            }
            for (auto& L : lanes_) {
                GumbelView gv = gum_;
                gv.state = L->d_gum.p;
                bool launched = false;
                int rc = L->net->simLaunchMz(L->pool, L->d_hidden.p, plan_.slab_slots, L->d_rootfeat.p, L->d_rootlegal.p, L->d_rootturn.p, games_[0].env->numPlayers(), L->d_policy.p,
                                            L->d_logit.p, L->d_value.p, L->d_reward.p, 0, 1, &launched, noise_cfg ? L->d_noise.p : nullptr,
                                            cfg_.actor_dirichlet_noise_epsilon, cfg_.actor_use_dirichlet_noise ? 1 : 2, plan_.dev_gumbel ? &gv : nullptr, L->pool.d_start_.p,
                                            host_gumbel, true, 0, false, plan_.sim_mode);
                if (rc) { return rc; }
                if (!launched) { const std::string why = mz_last_error(); setError("worker: the root expansion kernel was not launched (%s)", why.c_str()); return MZ_ERR_STATE; }
            }
            root_host_pending_ = false;
            sims_done_ = 0;
            sim0 = 1;
            trace_.add(16, nowMs() - t0);
        }
        const double tprep = nowMs();
        trace_.add(17, tprep - t0);
        // Cycles after this one join the launch while they need nothing from the host but RNG draws.  The cycle behind the root
        // expansion (sim index 1) needs the Dirichlet noise of the root children: its values only depend on the RNG stream and on
        // the NUMBER of root children = legal moves of the root position, which the host engine knows, so they are drawn here in the
        // reference's order ([noise][rotation] per actor, zero_actor.cpp:194-213 then :56) and applied by the kernel before simulation 1.
        const bool device_noise = cfg_.actor_use_dirichlet_noise || cfg_.actor_use_gumbel_noise; // the kernel applies either kind
        int batch = 1;
        while (i + batch < n && sim0 + batch < n_ + 1 && !(sim0 + batch == 1 && noise_cfg && !device_noise)) { ++batch; }
        // (root_on_device: the launch starts AT simulation 1, its noise is drawn right here)
        const bool noise_in_batch = noise_cfg && ((sim0 == 0 && batch > 1) || root_on_device);
        if (root_on_device && noise_cfg) { drawCycles(0, 1, 0); }
        // The launch goes out in up to three parts (mz_sim_split): simulation 0 needs no draw of this loop (its rotation was drawn in phase1), so it
        // runs while the host draws the root noise; a few simulations later the rest follows, whose rotation draws (AlphaZero: one per game and
        // simulation, 102 400 per move on BASELINE configs[1]) are made while the second part runs.  Same draws in the same order: nothing a record
        // could show.  The parts are queued back to back on the lane's stream; the draws of a later part travel on a second stream.
        const bool az_draws = desc_.type == 0 && cfg_.actor_use_random_rotation_features;
        int cuts[Lane::kSimParts + 1], pre_R[Lane::kSimParts] = {0}, parts = 1;
        bool pre_alt[Lane::kSimParts] = {false};
        for (int k = 0; k <= Lane::kSimParts; ++k) { cuts[k] = k == 0 ? 0 : batch; }
        if (cfg_.mz_sim_split && sim0 == 0 && batch > 1 && (noise_in_batch || az_draws)) {
            constexpr int kSecond = 16; // simulations of the middle part: 3 ms on BASELINE configs[1], three times what the draws of the rest take on this host
            cuts[parts++] = 1;
            if (az_draws && batch > 1 + kSecond && long(batch - 1 - kSecond) * G_ >= plan_.split_min_draws) { cuts[parts++] = 1 + kSecond; }
            cuts[parts] = batch;
        }
        // Gumbel rounds (mz_sim_rounds, muzero_atari): the launch is cut at the rounds whose leaves are evaluated ahead — [evaluation of the round's leaves]
        // [its simulations, which consume them in order] — with the stretches between them as ordinary parts; all queued back to back, no host step between
        // (muzero_atari: the launch starts at simulation 1, behind the device-side root expansion; MuZero board games: at simulation 0, the root's initial inference,
        // which goes out as a part of its own in front of the first round — a call that covers the whole move)
        const bool use_rounds = !rounds_.empty() && ((root_on_device && sim0 == 1) || (!plan_.sim_root_host && plan_.sim_mz && sim0 == 0 && batch == n_ + 1 && cfg_.mz_sim_split));
        if (use_rounds) {
            parts = 0;
            int at = 0; // offset inside the batch
            for (const Round& rd : rounds_) {
                const int o = rd.s0 - sim0;
                if (o < at || o + rd.R > batch || parts + 2 > Lane::kSimParts) { continue; }
                if (o > at) { cuts[parts] = at; pre_R[parts] = 0; ++parts; }
                cuts[parts] = o; pre_R[parts] = rd.R; pre_alt[parts] = rd.alt; ++parts;
                at = o + rd.R;
            }
            if (at < batch || parts == 0) { cuts[parts] = at; pre_R[parts] = 0; ++parts; }
            cuts[parts] = batch;
            for (auto& L : lanes_) { L->pre_epoch = L->net->nextPreEpoch(); }
        }
        int drawn = 1; // rows of the rotation table (= cycles of the batch) whose draws are made
        for (int part = 0; part < parts; ++part) {
            const int c0 = cuts[part], c1 = cuts[part + 1];
            if (drawn < c1) { drawCycles(drawn, c1, (noise_in_batch && !root_on_device) ? 1 : -1); drawn = c1; }
            for (auto& L : lanes_) {
                // the first part's uploads go in front of its kernel on the lane's stream (nothing is running); later ones overlap the running part
                hipStream_t us = part == 0 ? L->stream : L->up_stream;
                bool uploaded = false;
                if (desc_.type == 0 || part == 0) { MZ_HIP(hipMemcpyAsync(L->d_rot.p + size_t(c0) * L->n, L->h_rot.p + size_t(c0) * L->n, size_t(c1 - c0) * L->n, hipMemcpyHostToDevice, us)); uploaded = true; }
                if (noise_in_batch && (root_on_device ? part == 0 : (c0 <= 1 && 1 < c1))) { MZ_HIP(hipMemcpyAsync(L->d_noise.p, L->h_noise.p, size_t(L->n) * A_ * sizeof(float), hipMemcpyHostToDevice, us)); uploaded = true; }
                if (part > 0 && uploaded) {
                    MZ_HIP(hipEventRecord(L->ev_up, us));
                    MZ_HIP(hipStreamWaitEvent(L->stream, L->ev_up, 0));
                }
                bool launched = false;
                // Gumbel rounds: ONE pair of events around all parts — they are queued back to back without a host step, and an event between two dependent
                // launches costs ~10 us of idle GPU (12 of them per muzero_atari move); otherwise one pair per part: the host's draws between two parts are not kernel time
                if (!use_rounds || part == 0) { MZ_HIP(hipEventRecord(L->ev0[use_rounds ? 0 : part], L->stream)); }
                GumbelView gv = gum_;
                gv.state = L->d_gum.p;
                const int noise_kind = cfg_.actor_use_dirichlet_noise ? kNoiseDirichlet : kNoiseGumbel;
                const bool hg = host_gumbel && part == 0 && !root_on_device;
                if (use_rounds) {
                    // the first round needs the noisy logits before simulation 1 runs: the noise goes out as a launch of its own
                    if (sim0 + c0 == 1 && noise_in_batch) { int rcn = L->net->simRootNoiseMz(L->n); if (rcn) { return rcn; } }
                    if (pre_R[part] > 0) {
                        bool pre = false;
                        int rcp = MZ_OK;
                        if (cfg_.mz_sim_round_batch) {
                            rcp = L->net->simPreEvalBatchMz(L->n, L->pool.v_.max_depth, sim0 + c0, pre_R[part], L->pre_epoch, &pre, cfg_.mz_sim_round_leaves, pre_alt[part]);
                            if (pre) { ++stats_.pre_batch_launches; }
                        }
                        if (!rcp && !pre) { rcp = L->net->simPreEvalMz(L->n, L->pool.v_.max_depth, sim0 + c0, pre_R[part], L->pre_epoch, &pre, pre_alt[part] || !pairsUsable(), pairsUsable()); }
                        if (rcp) { return rcp; }
                        if (pre) { ++stats_.sim_launches; ++stats_.pre_launches; }
                    }
                }
                L->net->allowTailHelp(cfg_.mz_sim_round_pairs && plan_.lanes == 1); // (sim_help.h: only with the GPU to itself, one launch at a time)
                int rc = plan_.sim_mz ? L->net->simLaunchMz(L->pool, L->d_hidden.p, plan_.slab_slots, L->d_rootfeat.p, L->d_rootlegal.p, L->d_rootturn.p,
                                                      games_[0].env->numPlayers(), L->d_policy.p, L->d_logit.p, L->d_value.p, L->d_reward.p, sim0 + c0, c1 - c0,
                                                      &launched, noise_in_batch ? L->d_noise.p : nullptr, cfg_.actor_dirichlet_noise_epsilon, noise_kind,
                                                      plan_.dev_gumbel ? &gv : nullptr, L->pool.d_start_.p, hg, false, use_rounds ? L->pre_epoch : 0, use_rounds && noise_in_batch, plan_.sim_mode)
                                  : L->net->simLaunch(L->pool, L->godev.v_, L->d_policy.p, L->d_logit.p, L->d_value.p, L->d_rot.p + size_t(c0) * L->n, sim0 + c0, c1 - c0,
                                                     &launched, noise_in_batch ? L->d_noise.p : nullptr, cfg_.actor_dirichlet_noise_epsilon, noise_kind,
                                                     plan_.dev_gumbel ? &gv : nullptr, L->pool.d_start_.p, hg);
                if (rc) { return rc; }
                if (!launched) { const std::string why = mz_last_error(); setError("worker: the simulation kernel was not launched (%s)", why.c_str()); return MZ_ERR_STATE; }
                if (!use_rounds || part == parts - 1) { MZ_HIP(hipEventRecord(L->ev1[use_rounds ? 0 : part], L->stream)); }
                if (use_rounds && part == parts - 1 && L->h_prestat.p) { int rcc = L->net->simPreCountersAsync(L->h_prestat.p); if (rcc) { return rcc; } }
                ++stats_.sim_launches;
                // the launch that completes the move's search: the root statistics the per-move host logic reads next are queued right behind it
                L->rr_ahead = false;
                if (part == parts - 1 && sim0 + batch == n_ + 1 && !cfg_.mz_manual_step && L->pool.stream_ == L->stream) {
                    int rcr = L->pool.rootReadLaunch();
                    if (rcr) { return rcr; }
                    L->rr_ahead = true;
                }
            }
        }
        stats_.sim_cycles += batch;
        trace_.add(15, nowMs() - tprep);
        flushDeferred(); // the record strings of the move just decided: built while the launch runs
        sims_done_ = sim0 + batch - 1;
        pending_ = true;
        stats_.cycles += batch;
        stats_.leaf_evals += uint64_t(G_) * batch;
        i += batch;
        // the batch has to finish before the next host part (root statistics) or the return; its GPU time goes to ms_forward
        float ms_gpu = 0.0f;
        const double twait = nowMs();
        for (auto& L : lanes_) {
            MZ_HIP(hipStreamSynchronize(L->stream));
            float ms = 0.0f;
            for (int part = 0; part < (use_rounds ? 1 : parts); ++part) {
                float msp = 0.0f;
                MZ_HIP(hipEventElapsedTime(&msp, L->ev0[part], L->ev1[part]));
                ms += msp;
            }
            ms_gpu = std::max(ms_gpu, ms);
        }
        stats_.ms_forward += ms_gpu;
        if (use_rounds) { adaptRounds(); }
        stats_.ms_total += nowMs() - t0;
        trace_.add(18, nowMs() - twait);
    }
    for (auto& L : lanes_) {
        int rc = L->pool.checkError();
        if (rc) { return rc; }
    }
    return n;
}

// The lane's root statistics into the rr_* mirrors (the read every per-move decision starts from)
int Worker::thinkReadRoots(Lane& L)
{
    const int g0 = L.g0;
    const size_t o = size_t(g0) * A_;
    int rc = L.pool.rootRead(rr_nc_.data() + g0, rr_action_.data() + o, rr_count_.data() + o, rr_mean_.data() + o, rr_policy_.data() + o, rr_logit_.data() + o,
                             rr_noise_.data() + o, rr_value_.data() + o, rr_reward_.data() + o, rr_root_count_.data() + g0, rr_root_mean_.data() + g0,
                             rr_root_value_.data() + g0, rr_lo_.data() + g0, rr_hi_.data() + g0, rr_bsize_.data() + g0, false);
    if (rc) { return rc; }
    return L.pool.checkError();
}

// One step (ref zero_actor.cpp:129-157) of every game whose search is not done.  The host draws the step's rotations — game by game, each game's walks in order,
// also for the walks that turn out to be duplicates (:56 runs before :142) —, the device runs the step (think.h), and the host then does, game by game, what
// afterNNEvaluation does on the host's generator: the root noise behind the first step, the decision behind the step that completes the search.
int Worker::thinkCycle()
{
    const double t0 = nowMs();
    MZ_HIP(hipSetDevice(device_));
    Lane& L = *lanes_[0];
    const int B = thinkB_;
    uint8_t* rot = think_->hostRot();
    std::vector<int> bs(G_, 0);
    std::vector<uint8_t> expands_root(G_, 0);
    for (int g = 0; g < G_; ++g) {
        expands_root[g] = !think_done_[g] && think_count_[g] == 0;
        bs[g] = think_done_[g] ? 0 : std::min(B, n_ + 1 - think_count_[g]);
        for (int b = 0; b < bs[g]; ++b) { rot[size_t(g) * B + b] = cfg_.actor_use_random_rotation_features ? static_cast<uint8_t>(rngOf(g).randInt() % 8) : 0; }
    }
    int rc = think_->stepAsync(L.pool, L.godev.v_, *L.net);
    if (rc) { return rc; }
    MZ_HIP(hipStreamSynchronize(L.stream));
    if ((rc = L.pool.checkError())) { return rc; }
    const int* st = think_->hostStatus();
    bool first = false, finished = false;
    for (int g = 0; g < G_; ++g) {
        if (bs[g] == 0) { continue; }
        if (st[g * 4 + 1] != bs[g]) { setError("think: game %d walked %d times in a step of %d", g, st[g * 4 + 1], bs[g]); return MZ_ERR_STATE; }
        ++think_steps_; think_walks_ += bs[g]; think_queries_ += st[g * 4 + 2];
        stats_.leaf_evals += st[g * 4 + 2];
        think_rows_ += uint64_t(think_sym_) * st[g * 4 + 2];
        first = first || think_count_[g] == 0;
        think_count_[g] = st[g * 4 + 0];
        finished = finished || think_count_[g] == n_ + 1;
    }
    const bool want_noise = first && cfg_.actor_use_dirichlet_noise; // (a PUCT root: no Gumbel noise)
    if (want_noise || finished) {
        if ((rc = thinkReadRoots(L))) { return rc; }
    }
    std::vector<float>& noise = stream_noise_[0];
    bool all_done = true;
    for (int g = 0; g < G_; ++g) {
        if (want_noise) { noise_mask_[g] = expands_root[g]; }
        if (bs[g] != 0) {
            if (want_noise && expands_root[g]) { drawRootNoise(g, noise); } // the leaf was the root (zero_actor.cpp:95)
            if (think_count_[g] == n_ + 1) { // handleSearchDone() inside the last query's afterNNEvaluation (:96): its path still carries one virtual loss
                think_vl_child_[g] = st[g * 4 + 3] >= -1 ? st[g * 4 + 3] : -1;
                games_[g].selected = decideAction(g);
                handleSearchDone(g);
                think_vl_child_[g] = -2;
                think_done_[g] = 1;
            }
        }
        all_done = all_done && think_done_[g];
    }
    if (want_noise) {
        if ((rc = L.pool.rootSetNoise(noise_mask_.data(), noise_policy_.data(), noise_logit_.data(), noise_noise_.data()))) { return rc; }
        std::fill(noise_mask_.begin(), noise_mask_.end(), 1);
    }
    pending_ = true;
    ++stats_.cycles;
    if (all_done) { search_done_ = true; pending_ = false; }
    stats_.ms_total += nowMs() - t0;
    return MZ_OK;
}

int Worker::runCycles(int n)
{
    if (!ext_failed_.empty()) { setError("%s", ext_failed_.c_str()); return MZ_ERR_STATE; }
    if (!running_ || search_done_ || match_done_) { return 0; }
    if (think_) {
        for (int i = 0; i < n; ++i) {
            int rc = thinkCycle();
            if (rc) { return rc; }
            if (search_done_) { return i + 1; }
        }
        return n;
    }
    if (plan_.sim_kernel) { return runCyclesSim(n); }
    stop_now_ = false;
    for (int i = 0; i < n; ++i) {
        int rc = cycle();
        if (rc) { return rc; }
        if (stop_now_) { n = i; break; }
    }
    if (plan_.resident) { // the cycles above were only queued: the call returns when they have run
        const double t0 = nowMs();
        for (auto& L : lanes_) {
            MZ_HIP(hipStreamSynchronize(L->stream));
            int rc = L->pool.checkError();
            if (rc) { return rc; }
        }
        stats_.ms_total += nowMs() - t0;
    }
    return n;
}

int Worker::evaluatorBuffers(void** features, void** policy, void** logits, void** value) const
{
    if (!ext_) { setError("evaluator_buffers: the worker has a network of its own (not created by mz_worker_create_external)"); return MZ_ERR_STATE; }
    const mz_evaluator& ev = ext_->evaluator();
    if (features) { *features = ev.features; }
    if (policy) { *policy = const_cast<void*>(ev.policy); }
    if (logits) { *logits = const_cast<void*>(ev.logits); }
    if (value) { *value = const_cast<void*>(ev.value); }
    return MZ_OK;
}

int Worker::evaluatorLanePolicy(float* out, int capacity)
{
    if (!ext_) { setError("evaluator_lane_policy: the worker has a network of its own (not created by mz_worker_create_external)"); return MZ_ERR_STATE; }
    Lane& L = *lanes_[0];
    if (capacity < 0 || size_t(capacity) < L.d_policy.n) { setError("evaluator_lane_policy: buffer of %d floats, %zu needed", capacity, L.d_policy.n); return MZ_ERR_CAPACITY; }
    MZ_HIP(hipSetDevice(device_));
    MZ_HIP(hipStreamSynchronize(L.stream));
    MZ_HIP(hipMemcpy(out, L.d_policy.p, L.d_policy.n * sizeof(float), hipMemcpyDeviceToHost));
    return MZ_OK;
}

int Worker::popLine(char* buf, int cap)
{
    if (lines_.empty()) { return 0; }
    OutLine& front = *lines_.front();
    // Lines leave in order, complete.  A front line whose OBS tag is still being compressed is "none yet" (0), for the pop and for the size query: the caller
    // launches its next move instead of sleeping here (mz_worker_wait_lines is the call that blocks, for stop / quit / the end of a test)
    if (front.pending.load(std::memory_order_acquire) != 0) { return 0; }
    if (front.failed.load()) { // reported once: the line goes, the records behind it keep draining
        lines_.pop_front();
        setError("worker: building the OBS tag of a record failed (the record is dropped)");
        return MZ_ERR_STATE;
    }
    const std::string& s = front.text;
    const int len = static_cast<int>(s.size());
    if (!buf) { return len; } // size query: the line stays queued
    if (cap <= len) { setError("pop_line: buffer of %d bytes too small for a %d-byte line", cap, len); return MZ_ERR_CAPACITY; }
    memcpy(buf, s.data(), len);
    buf[len] = 0;
    lines_.pop_front();
    return len;
}

int Worker::waitLines() // until every queued line is complete; the number of queued lines
{
    if (obs_) { for (auto& l : lines_) { if (l->pending.load(std::memory_order_acquire) != 0) { obs_->wait(l.get()); } } }
    return static_cast<int>(lines_.size());
}

int Worker::searchAction(int g, int* action_id, int* player, int* resign) const
{
    if (g < 0 || g >= G_) { setError("search_action: game %d out of range", g); return MZ_ERR_ARG; }
    if (!search_done_) { setError("search_action: the search is not complete"); return MZ_ERR_STATE; }
    if (action_id) { *action_id = held_[g].action; }
    if (player) { *player = held_[g].player; }
    if (resign) { *resign = held_[g].resign ? 1 : 0; }
    return MZ_OK;
}

int Worker::actGame(int g, int action_id, int player) // BaseActor::act (ref base_actor.cpp:22-30)
{
    if (g < 0 || g >= G_) { setError("act: game %d out of range", g); return MZ_ERR_ARG; }
    if (!cfg_.mz_manual_step) { setError("act: the worker plays on its own (mz_manual_step=false)"); return MZ_ERR_STATE; }
    Game& gm = games_[g];
    if (!gm.env->act(action_id, player)) { return 0; }
    gm.action_info_history.resize(gm.env->actionIds().size());
    gm.action_info_history.back() = search_done_ ? held_[g].info : ActionInfo();
    // getActionInfo() runs AFTER env_.act() (base_actor.cpp:24-28): P and V are the completed search's, R is the reward of the move just played
    for (auto& kv : gm.action_info_history.back()) {
        if (kv.first == "R") { std::ostringstream oss; oss << gm.env->reward(); kv.second = oss.str(); }
    }
    ++stats_.moves;
    if (think_reuse_) { int rc = thinkReroot(g, action_id); if (rc) { return rc; } }
    return 1;
}

// The re-root of game g at `action` (think_reroot_kernel; the root's player is the one rootPlayerFor gives after the move: who played it).  action -1, or
// a move whose child is missing or unexpanded, leaves the empty tree reset_search starts from.  Runs on the lane's stream, behind everything queued, and waits.
int Worker::thinkReroot(int g, int action)
{
    if (!think_reuse_ || !think_) { return MZ_OK; }
    MZ_HIP(hipSetDevice(device_));
    int* a = think_->hostReroot();
    for (int i = (g < 0 ? 0 : g); i < (g < 0 ? G_ : g + 1); ++i) { a[i * 2] = action; a[i * 2 + 1] = rootPlayerFor(games_[i]); }
    int rc = think_->reroot(lanes_[0]->pool, lanes_[0]->godev.v_);
    if (rc) { return rc; }
    const int* st = think_->hostRerootStatus();
    for (int i = (g < 0 ? 0 : g); i < (g < 0 ? G_ : g + 1); ++i) {
        think_kept_[i] = st[i * 2];
        think_moved_[i] = 1;
        if (action >= 0) {
            ++reuse_reroots_;
            if (st[i * 2] > 0) { ++reuse_kept_; reuse_kept_visits_ += uint64_t(st[i * 2]); }
        }
    }
    return MZ_OK;
}

int Worker::resetSearchAll() // ZeroActor::resetSearch (ref zero_actor.cpp:29-34) of every game
{
    MZ_HIP(hipSetDevice(device_));
    for (auto& L : lanes_) { MZ_HIP(hipStreamSynchronize(L->stream)); }
    sims_done_ = 0;
    pending_ = false;
    search_done_ = false;
    root_host_pending_ = false;
    for (auto& h : held_) { h = Held(); }
    if (think_) {
        std::fill(think_count_.begin(), think_count_.end(), 0);
        std::fill(think_done_.begin(), think_done_.end(), 0);
        int rc = think_->clearAsync();
        if (rc) { return rc; }
        if (think_reuse_) { // a kept tree is searched on: its root's visits count towards n + 1 (isSearchDone unchanged)
            std::vector<uint8_t> mask(G_);
            for (int g = 0; g < G_; ++g) {
                mask[g] = think_kept_[g] > 0 ? 0 : 1;
                think_count_[g] = think_kept_[g];
                think_done_[g] = think_kept_[g] >= n_ + 1 ? 1 : 0;
                think_kept_[g] = 0;
                think_moved_[g] = 0;
            }
            return resetAllSearches(mask.data());
        }
    }
    return resetAllSearches();
}

// ZeroActor::think's `if (!isSearchDone()) { handleSearchDone(); }` (ref zero_actor.cpp:40-45): the search stops where it stands — at least the root has to be
// expanded — and the decision is taken from the simulations run so far (move decision, resign test, P / V strings: exactly what the complete search's last
// cycle does, with fewer visits).  Per-actor stepping only.
int Worker::finishSearch()
{
    if (!cfg_.mz_manual_step) { setError("finish_search: the worker plays on its own (mz_manual_step=false)"); return MZ_ERR_STATE; }
    if (search_done_) { return MZ_OK; }
    if (think_) { // between two steps no virtual loss is outstanding: the games that are not done decide on the plain statistics, the others keep their decision
        for (int g = 0; g < G_; ++g) {
            if (think_count_[g] < 1) { setError("finish_search: the root has not been evaluated yet (run at least one step of the search first)"); return MZ_ERR_STATE; }
        }
        MZ_HIP(hipSetDevice(device_));
        int rc = thinkReadRoots(*lanes_[0]);
        if (rc) { return rc; }
        for (int g = 0; g < G_; ++g) {
            if (think_done_[g]) { continue; }
            games_[g].selected = decideAction(g);
            handleSearchDone(g);
            think_done_[g] = 1;
        }
        search_done_ = true;
        pending_ = false;
        return MZ_OK;
    }
    if (!pending_ || sims_done_ < 1) { setError("finish_search: the root has not been evaluated yet (run at least two cycles of the search first)"); return MZ_ERR_STATE; }
    MZ_HIP(hipSetDevice(device_));
    sim_pre_ = sims_done_;
    sim_post_ = sims_done_ + 1;
    const bool host_gumbel = plan_.dev_gumbel;
    for (auto& L : lanes_) {
        int rc = MZ_OK;
        MZ_HIP(hipStreamSynchronize(L->stream));
        if (host_gumbel && (rc = syncGumbel(*L, false))) { return rc; }
        if ((rc = phase1(*L, false, true, false))) { return rc; } // done = true: root statistics, decision, held action (manual stepping returns before the next selection)
    }
    root_host_pending_ = false;
    search_done_ = true;
    pending_ = false;
    sims_done_ = 0;
    return MZ_OK;
}

int Worker::resetGameAt(int g) // ZeroActor::reset without the search part (ref zero_actor.cpp:23-27, base_actor.cpp:8-13)
{
    if (g < 0 || g >= G_) { setError("reset_game: game %d out of range", g); return MZ_ERR_ARG; }
    resetGame(games_[g], rngOf(g));
    return thinkReroot(g, -1);
}

int Worker::emitGame(int g) // ThreadSharedData::outputGame (ref actor_group.cpp:24-50)
{
    if (g < 0 || g >= G_) { setError("emit_game: game %d out of range", g); return MZ_ERR_ARG; }
    flushDeferred();
    outputGame(games_[g]);
    return MZ_OK;
}

int Worker::envQuery(int g, int what, float* out) const
{
    if (g < 0 || g >= G_ || !out) { setError("env_query: bad arguments"); return MZ_ERR_ARG; }
    const GameEnv& e = *games_[g].env;
    switch (what) {
        case 0: *out = e.isTerminal() ? 1.0f : 0.0f; break;
        case 1: *out = static_cast<float>(e.turn()); break;
        case 2: *out = e.evalScore(false); break;
        case 3: *out = e.evalScore(true); break;
        case 4: *out = static_cast<float>(e.actionIds().size()); break;
        case 5: *out = e.reward(); break;
        default: setError("env_query: unknown query %d", what); return MZ_ERR_ARG;
    }
    return MZ_OK;
}

// BaseActor::act(const std::vector<std::string>&) (ref base_actor.cpp:32-40 -> Env::act(action_string_args), base_env.h:326-333 / atari.cpp:24-39)
int Worker::actString(int g, const char* const* args, int nargs)
{
    if (g < 0 || g >= G_) { setError("act: game %d out of range", g); return MZ_ERR_ARG; }
    if (nargs != 2 || !args || !args[0] || !args[1] || strlen(args[0]) != 1) { setError("act: expected {player char, action string} (ref base_env.h:328-329)"); return MZ_ERR_ARG; }
    const char c = args[0][0]; // charToPlayer (ref base_env.cpp:15-25)
    const int player = (c == 'B' || c == 'b') ? 1 : (c == 'W' || c == 'w') ? 2 : 0;
    const int action = games_[g].env->actionFromString(args[1]);
    if (player == 0 || action < 0 || action >= A_) { return 0; } // not an action of this game: act() fails like an illegal move
    return actGame(g, action, player);
}

// BaseActor::getActionInfoHistory() (ref base_actor.h:33-34): per move its (key, value) pairs.  Serialised as moves joined by '\x1e', inside a move
// key '\x1f' value '\x1f' ... (neither byte can occur in a tag: the values are numbers, "id:count" lists or hex)
int Worker::actionInfoHistory(int g, char* buf, int cap)
{
    if (g < 0 || g >= G_) { setError("action_info_history: game %d out of range", g); return MZ_ERR_ARG; }
    flushDeferred();
    std::string s;
    const auto& h = games_[g].action_info_history;
    for (size_t i = 0; i < h.size(); ++i) {
        if (i) { s += '\x1e'; }
        for (const auto& kv : h[i]) { s += kv.first; s += '\x1f'; s += kv.second; s += '\x1f'; }
    }
    const int len = static_cast<int>(s.size());
    if (!buf) { return len; }
    if (cap <= len) { setError("action_info_history: buffer of %d bytes too small for %d", cap, len); return MZ_ERR_CAPACITY; }
    memcpy(buf, s.data(), len);
    buf[len] = 0;
    return len;
}

int Worker::envFeatures(int g, int rotation, float* out, int capacity) const // Env::getFeatures(rotation) (ref base_env.h:88)
{
    if (g < 0 || g >= G_ || rotation < 0 || rotation > 7) { setError("env_features: bad arguments"); return MZ_ERR_ARG; }
    const int n = games_[g].env->featureSize();
    if (!out) { return n; }
    if (capacity < n) { setError("env_features: %d floats needed", n); return MZ_ERR_CAPACITY; }
    games_[g].env->features(rotation, out);
    return n;
}

int Worker::envLegalMask(int g, uint8_t* out, int capacity) const // Env::isLegalAction / getLegalActions for the player to move
{
    if (g < 0 || g >= G_ || !out || capacity < A_) { setError("env_legal_mask: bad arguments (%d bytes needed)", A_); return MZ_ERR_ARG; }
    games_[g].env->legalMask(out);
    return A_;
}

int Worker::envSetTurn(int g, int player) // Env::setTurn (ref base_env.h:103)
{
    if (g < 0 || g >= G_ || player < 1 || player > games_[g].env->numPlayers()) { setError("env_set_turn: bad arguments"); return MZ_ERR_ARG; }
    if (!cfg_.mz_manual_step) { setError("env_set_turn: the worker plays on its own (mz_manual_step=false)"); return MZ_ERR_STATE; }
    games_[g].env->setTurn(player);
    return thinkReroot(g, -1);
}

int Worker::envResetSeed(int g, int seed) // Env::reset(seed) (ref atari.h:55; console.cpp:289): the seed comes from the caller, no draw
{
    if (g < 0 || g >= G_) { setError("env_reset_seed: game %d out of range", g); return MZ_ERR_ARG; }
    if (!cfg_.mz_manual_step) { setError("env_reset_seed: the worker plays on its own (mz_manual_step=false)"); return MZ_ERR_STATE; }
    games_[g].env->resetSeed(seed);
    games_[g].action_info_history.clear();
    return thinkReroot(g, -1);
}

int Worker::envRotateAction(int g, int action_id, int rotation) const // Env::getRotateAction (ref base_env.h:99)
{
    if (g < 0 || g >= G_ || action_id < 0 || action_id >= A_ || rotation < 0 || rotation > 7) { setError("env_rotate_action: bad arguments"); return MZ_ERR_ARG; }
    const RotationTables* r = games_[g].env->rot();
    return r ? r->fwd[rotation][action_id] : action_id; // the Atari-shaped env has no rotations (ref atari.h:77-78)
}

int Worker::peekRecord(int game, char* buf, int cap, const char* const* keys, const char* const* values, int ntags)
{
    if (game < 0 || game >= G_) { setError("peek_record: game %d out of range", game); return MZ_ERR_ARG; }
    flushDeferred();
    ActionInfo extra;
    if (match_) { extra.push_back({"PB", matchName(games_[game].m_first_side)}); extra.push_back({"PW", matchName(1 - games_[game].m_first_side)}); }
    for (int i = 0; i < ntags; ++i) { extra.push_back({keys[i], values[i]}); }
    const std::string s = record(games_[game], extra);
    const int len = static_cast<int>(s.size());
    if (!buf) { return len; } // size query
    if (cap <= len) { setError("peek_record: buffer of %d bytes too small for a %d-byte record", cap, len); return MZ_ERR_CAPACITY; }
    memcpy(buf, s.data(), len);
    buf[len] = 0;
    return len;
}

// The read-out of game g's visited tree.  Valid under mz_manual_step at every return of mz_worker_run_cycles — mid-search, after the last cycle, after
// finish_search, until reset_search starts the next search —, also under the batched think (between two steps no virtual loss is outstanding).  It reports what
// the pool holds and changes nothing: one kernel and three copies on the lane's stream, behind whatever the last cycle queued.
int Worker::treeSnapshot(int g, TreeSnapshot* out)
{
    if (g < 0 || g >= G_) { setError("tree: game %d out of range", g); return MZ_ERR_ARG; }
    if (!cfg_.mz_manual_step) { setError("tree: the worker plays on its own (mz_manual_step=false)"); return MZ_ERR_STATE; }
    Lane& L = laneOf(g);
    if (!L.tree) {
        if (!createTreeReader) { setError("tree: this build has no device code for the read-out"); return MZ_ERR_DEVICE; }
        std::unique_ptr<TreeReader> r(createTreeReader());
        int rc = r->init(device_, L.stream, L.pool, n_ + 2); // n + 1 simulations visit at most n + 1 nodes besides the root
        if (rc) { return rc; }
        L.tree = std::move(r);
    }
    return L.tree->read(L.pool, g - L.g0, out);
}

namespace {

std::string nodeText(const TreeSnapshot& t, int e) // MCTSNode::toString (ref mcts.cpp:63-75)
{
    std::ostringstream oss;
    oss.precision(4);
    oss << std::fixed << "p = " << t.frow(kTrPolicy)[e] << ", p_logit = " << t.frow(kTrLogit)[e] << ", p_noise = " << t.frow(kTrNoise)[e] << ", v = " << t.frow(kTrValue)[e]
        << ", r = " << t.frow(kTrReward)[e] << ", mean = " << t.frow(kTrMean)[e] << ", count = " << t.frow(kTrCount)[e];
    return oss.str();
}

int copyOut(const std::string& s, char* buf, int cap, const char* what)
{
    const int len = static_cast<int>(s.size());
    if (!buf) { return len; } // size query
    if (cap <= len) { setError("%s: buffer of %d bytes too small for %d", what, cap, len); return MZ_ERR_CAPACITY; }
    memcpy(buf, s.data(), len);
    buf[len] = 0;
    return len;
}

} // namespace

// Tree::toString(env_string) (ref tree.h:79-110) from the read-out.  The kept children of an entry are contiguous and in child order, so the recursion of
// getTreeInfo_r is a walk over [first[e], first[e + 1]).  An expanded child has been visited, so it is among the kept ones: isLeaf() can be counted there.
int Worker::treeString(int g, char* buf, int cap)
{
    TreeSnapshot t;
    int rc = treeSnapshot(g, &t);
    if (rc) { return rc; }
    flushDeferred();
    const std::string env_string = record(games_[g], ActionInfo());
    const int n = t.entries;
    const int *parent = t.irow(kTrParent), *action = t.irow(kTrAction), *player = t.irow(kTrPlayer), *nc = t.irow(kTrNumChildren);
    std::vector<int> first(n + 1, n), expanded(n, 0);
    for (int e = n - 1; e >= 1; --e) { first[parent[e]] = e; if (nc[e] > 0) { ++expanded[parent[e]]; } }
    for (int e = n - 1; e >= 0; --e) { if (first[e] == n) { first[e] = first[e + 1]; } } // no kept children: an empty range
    std::ostringstream oss;
    oss << env_string.substr(0, env_string.size() - 1) << "C[" << nodeText(t, 0) << "]";
    // the recursion without the stack of calls: (entry, next child, end)
    struct Frame { int e, c, end; };
    std::vector<Frame> st;
    st.push_back({0, first[0], first[1]});
    while (!st.empty()) {
        Frame& f = st.back();
        const bool paren = expanded[f.e] > 1;
        if (f.c > first[f.e] && paren) { oss << ")"; } // the child before this one is complete
        if (f.c == f.end) { st.pop_back(); continue; }
        const int c = f.c++;
        if (paren) { oss << "("; }
        oss << (player[c] == 0 ? 'N' : player[c] == 1 ? 'B' : player[c] == 2 ? 'W' : '?') << "[" << action[c] << "]C[" << nodeText(t, c) << "]";
        st.push_back({c, first[c], first[c + 1]});
    }
    oss << ")";
    return copyOut(oss.str(), buf, cap, "tree_string");
}

// which = 0: the root node's text; 1: the text of the node the decision chose (selected_node_, ref zero_actor.cpp:173-174), once the search is done
int Worker::nodeInfo(int g, int which, char* buf, int cap)
{
    if (which != 0 && which != 1) { setError("node_info: which = %d (0 root, 1 action node)", which); return MZ_ERR_ARG; }
    TreeSnapshot t;
    int rc = treeSnapshot(g, &t);
    if (rc) { return rc; }
    if (which == 0) { return copyOut(nodeText(t, 0), buf, cap, "node_info"); }
    if (!search_done_) { setError("node_info: the search is not complete"); return MZ_ERR_STATE; }
    if (think_reuse_ && think_moved_[g]) { setError("node_info: the tree of game %d was re-rooted by a move since its decision (mz_think_reuse_tree=true): the chosen node is no root child any more", g); return MZ_ERR_STATE; }
    const int sel = games_[g].selected;
    for (int e = 1; e < t.entries && t.irow(kTrParent)[e] == 0; ++e) {
        if (t.irow(kTrOrdinal)[e] == sel) { return copyOut(nodeText(t, e), buf, cap, "node_info"); }
    }
    setError("node_info: the chosen root child %d of game %d has no visits and is not read back", sel, g);
    return MZ_ERR_STATE;
}

// load_model with the file's content in hand (Network::loadModel of every network of this worker, ref actor_group.cpp:227-232, network.h:18-37)
int Worker::loadModel(const std::string& path, const mz_net_desc& file_desc, const float* weights, size_t count)
{
    if (external_) { cfg_.nn_file_name = path; return MZ_OK; } // the weights are the caller's: the actor only follows the name (EV tag)
    if (match_) { return matchFixed("load_model"); }
    MZ_HIP(hipSetDevice(device_));
    mz_net_desc a = file_desc, b = desc_;
    a.game_name[sizeof(a.game_name) - 1] = 0;
    memset(a.game_name, 0, sizeof(a.game_name)); // (the game's name is the trainer's label, not a shape)
    memset(b.game_name, 0, sizeof(b.game_name));
    if (memcmp(&a, &b, sizeof(a)) != 0) {
        setError("load_model %s: the file's hyper-parameters are not those of the running network (%s, %d blocks x %d channels)", path.c_str(),
                 desc_.game_name, desc_.num_blocks, desc_.num_hidden_channels);
        return MZ_ERR_ARG;
    }
    if (!shared_net_) {
        for (auto& L : lanes_) {
            MZ_HIP(hipStreamSynchronize(L->stream));
            int rc = L->net->reload(weights, count);
            if (rc) { return rc; }
        }
    }
    cfg_.nn_file_name = path;
    return thinkReroot(-1, -1); // (mz_think_reuse_tree) a kept tree holds the old network's outputs
}

int Worker::command(const std::string& line) // ref actor_group.cpp:200-252
{
    const std::string prefix = line.substr(0, line.find(' '));
    std::istringstream ign(cfg_.zero_actor_ignored_command);
    std::string tok;
    while (ign >> tok) { if (tok == prefix) { return MZ_OK; } }
    MZ_HIP(hipSetDevice(device_));
    if (prefix == "start") { running_ = true; }
    else if (prefix == "stop") { running_ = false; }
    else if (prefix == "reset_actors") {
        if (match_) { setError("reset_actors: the games of a match follow its schedule from step 0 (a new match is a new worker)"); return MZ_ERR_STATE; }
        for (auto& gm : games_) { resetGame(gm, main_rng_); } // handleCommand runs on the main thread (actor_group.cpp:200-219)
        sims_done_ = 0;
        pending_ = false;
        for (auto& L : lanes_) { MZ_HIP(hipStreamSynchronize(L->stream)); }
        if (think_reuse_) { std::fill(think_kept_.begin(), think_kept_.end(), 0); }
        return resetAllSearches();
    } else if (prefix == "load_model") {
        if (line.find(' ') == std::string::npos) { setError("load_model needs a path"); return MZ_ERR_ARG; }
        const std::string path = line.substr(line.find(' ') + 1);
        if (match_) { return matchFixed("load_model"); }
        if (shared_net_ || external_) { // the caller's Network::loadModel has (or will have) reloaded the weights; the actor only follows the name (EV tag)
            pending_weights_.clear();
            cfg_.nn_file_name = path;
            return thinkReroot(-1, -1);
        }
        if (pending_weights_.empty()) { // the reference's path: every network re-reads the file (actor_group.cpp:227-232)
            mz_net_desc nd;
            std::vector<float> file;
            if (!readWeightFile(path, &nd, &file)) { return MZ_ERR_ARG; }
            return loadModel(path, nd, file.data(), file.size());
        }
        std::vector<float> staged;
        staged.swap(pending_weights_);
        return loadModel(path, desc_, staged.data(), staged.size());
    } else if (prefix == "update_config") {
        if (line.find(' ') == std::string::npos) { setError("update_config needs a configuration string"); return MZ_ERR_ARG; }
        WorkerConfig nc = cfg_;
        if (!nc.loadFromString(line.substr(line.find(' ') + 1))) { return MZ_ERR_ARG; }
        // keys whose values were turned into device state when the worker was created (pool and slab sizes, PUCT tables, Gumbel constants,
        // kernels, engines): a live change would leave host and device disagreeing, so it is refused by name
        const char* fixed = nullptr;
#define MZ_FIXED(k) if (!fixed && !(nc.k == cfg_.k)) { fixed = #k; }
        MZ_FIXED(actor_num_simulation) MZ_FIXED(actor_mcts_puct_base) MZ_FIXED(actor_mcts_puct_init) MZ_FIXED(actor_mcts_reward_discount)
        MZ_FIXED(actor_mcts_value_rescale) MZ_FIXED(actor_mcts_value_flipping_player) MZ_FIXED(actor_use_gumbel) MZ_FIXED(actor_gumbel_sample_size)
        MZ_FIXED(actor_gumbel_sigma_visit_c) MZ_FIXED(actor_gumbel_sigma_scale_c) MZ_FIXED(zero_num_threads) MZ_FIXED(zero_num_parallel_games)
        MZ_FIXED(nn_type_name) MZ_FIXED(env_board_size) MZ_FIXED(env_go_komi) MZ_FIXED(env_go_ko_rule) MZ_FIXED(env_game) MZ_FIXED(atari_init_q)
        MZ_FIXED(env_atari_name) MZ_FIXED(env_atari_episode_length) MZ_FIXED(mz_pipeline_lanes) MZ_FIXED(mz_rng_streams) MZ_FIXED(mz_cpu_base) MZ_FIXED(mz_signal_wait)
        MZ_FIXED(mz_sim_kernel) MZ_FIXED(mz_sim_cluster) MZ_FIXED(mz_sim_split) MZ_FIXED(mz_sim_rounds) MZ_FIXED(mz_sim_round_min) MZ_FIXED(mz_sim_round_alt) MZ_FIXED(mz_sim_round_batch) MZ_FIXED(mz_sim_rounds_board) MZ_FIXED(mz_sim_round_pairs) MZ_FIXED(mz_sim_round_leaves) MZ_FIXED(mz_manual_step) MZ_FIXED(mz_nn_precision) MZ_FIXED(mz_raw_observations) MZ_FIXED(mz_device_env) MZ_FIXED(mz_zero_copy) MZ_FIXED(mz_think_reuse_tree) MZ_FIXED(mz_think_symmetries)
        // a match's length, names and arithmetic are part of its records and its tally from step 0 (every other worker never reads the five keys)
        MZ_FIXED(mz_match_games) MZ_FIXED(mz_match_name_a) MZ_FIXED(mz_match_name_b) MZ_FIXED(mz_match_precision_a) MZ_FIXED(mz_match_precision_b)
        if (match_) { MZ_FIXED(zero_actor_intermediate_sequence_length) }
        // the Atari-shaped environments keep a window of screens sized from these three at creation (ref atari.cpp:87); records of a larger window
        // would miss frames, so they are fixed where observations are kept (board games: free to change, like the reference)
        if (games_[0].env->hasObservations()) { MZ_FIXED(zero_actor_intermediate_sequence_length) MZ_FIXED(learner_n_step_return) MZ_FIXED(learner_muzero_unrolling_step) }
        // Gomoku's rules live in its engines (host and device) from creation; for every other game the two keys are inert
        if (gameFromName(cfg_.env_game.c_str()) == kGomoku) { MZ_FIXED(env_gomoku_rule) MZ_FIXED(env_gomoku_exactly_five_stones) }
        // ... and so does Hex's swap rule
        if (gameFromName(cfg_.env_game.c_str()) == kHex) { MZ_FIXED(env_hex_use_swap_rule) }
        if (gameFromName(cfg_.env_game.c_str()) == kHavannah) { MZ_FIXED(env_havannah_use_swap_rule) }
#undef MZ_FIXED
        if (fixed) { setError("update_config: %s is fixed when the worker is created (restart the worker to change it)", fixed); return MZ_ERR_ARG; }
        cfg_ = nc;
    } else if (prefix == "quit") {
        running_ = false;
        return 1;
    }
    return MZ_OK; // anything else (keep_alive, ...) is silently ignored
}

} // namespace mz

// ------------------------------------------------------------------------------------------------
struct mz_worker { mz::Worker w; };
struct mz_net { mz::Net net; };
struct mz_env { std::unique_ptr<mz::GameEnv> e; };

static int envdevPlayout(int device, mz::GameEnv* env, float komi, const int* actions, int count, int root_prefix, const int* rots, uint32_t* feat_out,
                         uint8_t* legal_out, int* terminal_out, float* eval_out, int* player_out);

extern "C" {

int mz_usable_cpus(void) { return mz::usableCpus(); }

mz_worker* mz_worker_create(int device, const char* conf, const mz_net_desc* desc, const float* weights, size_t count)
{
    if (!conf || (!desc != !weights)) { mz::setError("mz_worker_create: NULL argument"); return nullptr; }
    std::unique_ptr<mz_worker> w(new mz_worker());
    mz_net_desc file_desc;
    std::vector<float> file_weights;
    if (!desc) { // the network comes from the configuration's nn_file_name (ref actor_group.cpp:168-177)
        mz::WorkerConfig c;
        if (!c.loadFromString(conf)) { return nullptr; }
        if (c.nn_file_name.empty()) { mz::setError("mz_worker_create: no network given and nn_file_name is empty"); return nullptr; }
        if (!mz::readWeightFile(c.nn_file_name, &file_desc, &file_weights)) { return nullptr; }
        desc = &file_desc;
        weights = file_weights.data();
        count = file_weights.size();
    }
    if (w->w.init(device, conf, *desc, weights, count) != MZ_OK) { return nullptr; }
    return w.release();
}
mz_worker* mz_worker_create_shared(int device, const char* conf, mz_net* net)
{
    if (!conf || !net) { mz::setError("mz_worker_create_shared: NULL argument"); return nullptr; }
    std::unique_ptr<mz_worker> w(new mz_worker());
    if (w->w.init(device, conf, net->net.desc_, nullptr, 0, &net->net) != MZ_OK) { return nullptr; }
    return w.release();
}
mz_worker* mz_worker_create_external(int device, const char* conf, const mz_net_desc* desc, const mz_evaluator* ev)
{
    if (!conf || !desc || !ev) { mz::setError("mz_worker_create_external: NULL argument"); return nullptr; }
    std::unique_ptr<mz_worker> w(new mz_worker());
    if (w->w.init(device, conf, *desc, nullptr, 0, nullptr, ev) != MZ_OK) { return nullptr; }
    return w.release();
}
mz_worker* mz_worker_create_match(int device, const char* conf, const mz_net_desc* desc, const float* weights_a, size_t count_a, const float* weights_b, size_t count_b)
{
    if (!conf || !desc || !weights_a || !weights_b) { mz::setError("mz_worker_create_match: NULL argument"); return nullptr; }
    std::unique_ptr<mz_worker> w(new mz_worker());
    if (w->w.initMatch(device, conf, *desc, weights_a, count_a, weights_b, count_b) != MZ_OK) { return nullptr; }
    return w.release();
}
int mz_worker_match_stats(mz_worker* w, mz_match_stats* out)
{
    if (!w || !out) { mz::setError("mz_worker_match_stats: NULL argument"); return MZ_ERR_ARG; }
    return w->w.matchStats(out);
}
int mz_worker_evaluator_buffers(mz_worker* w, void** features, void** policy, void** logits, void** value)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.evaluatorBuffers(features, policy, logits, value);
}
int mz_worker_evaluator_lane_policy(mz_worker* w, float* out, int capacity)
{
    if (!w || !out) { mz::setError("mz_worker_evaluator_lane_policy: NULL argument"); return MZ_ERR_ARG; }
    return w->w.evaluatorLanePolicy(out, capacity);
}
int mz_worker_cycles_per_move(const mz_worker* w) { return w ? w->w.cyclesPerMove() : MZ_ERR_ARG; }
int mz_worker_lanes(const mz_worker* w) { return w ? w->w.numLanes() : MZ_ERR_ARG; }
void mz_worker_destroy(mz_worker* w) { delete w; }
int mz_worker_command(mz_worker* w, const char* line)
{
    if (!w || !line) { mz::setError("mz_worker_command: NULL argument"); return MZ_ERR_ARG; }
    return w->w.command(line);
}
int mz_worker_load_model(mz_worker* w, const char* path, const mz_net_desc* desc, const float* weights, size_t count)
{
    if (!w || !path || !desc || !weights) { mz::setError("mz_worker_load_model: NULL argument"); return MZ_ERR_ARG; }
    return w->w.loadModel(path, *desc, weights, count);
}
int mz_worker_set_weights(mz_worker* w, const float* weights, size_t count)
{
    if (!w || !weights) { mz::setError("mz_worker_set_weights: NULL argument"); return MZ_ERR_ARG; }
    return w->w.setWeights(weights, count);
}
int mz_worker_run_cycles(mz_worker* w, int n)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.runCycles(n);
}
int mz_worker_pop_line(mz_worker* w, char* buf, int cap)
{
    if (!w) { mz::setError("NULL argument"); return MZ_ERR_ARG; }
    return w->w.popLine(buf, cap);
}
int mz_worker_wait_lines(mz_worker* w)
{
    if (!w) { mz::setError("NULL argument"); return MZ_ERR_ARG; }
    return w->w.waitLines();
}
int mz_worker_peek_record(mz_worker* w, int game, char* buf, int cap)
{
    if (!w) { mz::setError("NULL argument"); return MZ_ERR_ARG; }
    return w->w.peekRecord(game, buf, cap);
}
int mz_worker_tree_size(mz_worker* w, int game)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    mz::TreeSnapshot t;
    int rc = w->w.treeSnapshot(game, &t);
    return rc ? rc : t.entries;
}
int mz_worker_tree(mz_worker* w, int game, int cap, int* parent, int* ordinal, int* action, int* player, int* num_children, int* depth, float* count, float* mean,
                   float* policy, float* logit, float* noise, float* value, float* reward)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    mz::TreeSnapshot t;
    int rc = w->w.treeSnapshot(game, &t);
    if (rc) { return rc; }
    if (cap < t.entries) { mz::setError("tree: buffers of %d entries, %d needed", cap, t.entries); return MZ_ERR_CAPACITY; }
    int* io[mz::kTreeInts] = {parent, ordinal, action, player, num_children, depth};
    float* fo[mz::kTreeFloats] = {count, mean, policy, logit, noise, value, reward};
    for (int r = 0; r < mz::kTreeInts; ++r) { if (io[r]) { memcpy(io[r], t.irow(r), t.entries * sizeof(int)); } }
    for (int r = 0; r < mz::kTreeFloats; ++r) { if (fo[r]) { memcpy(fo[r], t.frow(r), t.entries * sizeof(float)); } }
    return t.entries;
}
int mz_worker_tree_string(mz_worker* w, int game, char* buf, int cap)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.treeString(game, buf, cap);
}
int mz_worker_node_info(mz_worker* w, int game, int which, char* buf, int cap)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.nodeInfo(game, which, buf, cap);
}
int mz_worker_record(mz_worker* w, int game, const char* const* keys, const char* const* values, int ntags, char* buf, int cap)
{
    if (!w || ntags < 0 || (ntags > 0 && (!keys || !values))) { mz::setError("mz_worker_record: bad arguments"); return MZ_ERR_ARG; }
    return w->w.peekRecord(game, buf, cap, keys, values, ntags);
}
int mz_worker_search_done(const mz_worker* w) { return w ? (w->w.searchDone() ? 1 : 0) : MZ_ERR_ARG; }
int mz_worker_search_action(const mz_worker* w, int game, int* action_id, int* player, int* is_resign)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.searchAction(game, action_id, player, is_resign);
}
int mz_worker_act(mz_worker* w, int game, int action_id, int player)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.actGame(game, action_id, player);
}
int mz_worker_reset_search(mz_worker* w)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.resetSearchAll();
}
int mz_worker_finish_search(mz_worker* w)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.finishSearch();
}
int mz_worker_reset_game(mz_worker* w, int game)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.resetGameAt(game);
}
int mz_worker_emit_game(mz_worker* w, int game)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.emitGame(game);
}
int mz_worker_env_query(const mz_worker* w, int game, int what, float* out)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.envQuery(game, what, out);
}
int mz_worker_act_string(mz_worker* w, int game, const char* const* args, int nargs)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.actString(game, args, nargs);
}
int mz_worker_action_info_history(mz_worker* w, int game, char* buf, int cap)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.actionInfoHistory(game, buf, cap);
}
int mz_worker_env_features(const mz_worker* w, int game, int rotation, float* out, int capacity)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.envFeatures(game, rotation, out, capacity);
}
int mz_worker_env_legal_mask(const mz_worker* w, int game, uint8_t* out, int capacity)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.envLegalMask(game, out, capacity);
}
int mz_worker_env_set_turn(mz_worker* w, int game, int player)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.envSetTurn(game, player);
}
int mz_worker_env_reset_seed(mz_worker* w, int game, int seed)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.envResetSeed(game, seed);
}
int mz_worker_env_rotate_action(const mz_worker* w, int game, int action_id, int rotation)
{
    if (!w) { mz::setError("NULL worker"); return MZ_ERR_ARG; }
    return w->w.envRotateAction(game, action_id, rotation);
}
int mz_worker_think_reuse_stats(mz_worker* w, uint64_t* reroots, uint64_t* kept, uint64_t* kept_visits)
{
    if (!w) { mz::setError("think_reuse_stats: NULL argument"); return MZ_ERR_ARG; }
    return w->w.thinkReuseStats(reroots, kept, kept_visits);
}
int mz_worker_think_symmetry_stats(const mz_worker* w, long long* queries, long long* rows)
{
    if (!w) { mz::setError("think_symmetry_stats: NULL argument"); return MZ_ERR_ARG; }
    return w->w.thinkSymmetryStats(queries, rows);
}
int mz_worker_think_stats(mz_worker* w, uint64_t* steps, uint64_t* walks, uint64_t* queries)
{
    if (!w) { mz::setError("think_stats: NULL argument"); return MZ_ERR_ARG; }
    return w->w.thinkStats(steps, walks, queries);
}
int mz_worker_get_stats(mz_worker* w, mz_worker_stats* out)
{
    if (!w || !out) { return MZ_ERR_ARG; }
    return w->w.getStats(out);
}
mz_net* mz_worker_net(mz_worker* w) { return w ? reinterpret_cast<mz_net*>(w->w.netOrNull()) : nullptr; } // NULL on an external evaluator and on a match

mz_env* mz_env_create(const char* conf)
{
    mz::WorkerConfig c;
    if (!conf || !c.loadFromString(conf)) { return nullptr; }
    std::unique_ptr<mz_env> e(new mz_env());
    e->e = mz::createGameEnv(mz::envOptions(c, 108001));
    if (!e->e) { return nullptr; }
    return e.release();
}
void mz_env_destroy(mz_env* e) { delete e; }
void mz_env_reset(mz_env* e) { e->e->reset(); }
void mz_env_reset_seed(mz_env* e, int seed) { e->e->resetSeed(seed); }
float mz_env_reward(const mz_env* e) { return e->e->reward(); }
int mz_env_act(mz_env* e, int action_id, int player) { return e->e->act(action_id, player) ? 1 : 0; }
int mz_env_turn(const mz_env* e) { return e->e->turn(); }
int mz_env_is_terminal(const mz_env* e) { return e->e->isTerminal() ? 1 : 0; }
float mz_env_eval_score(const mz_env* e, int is_resign) { return e->e->evalScore(is_resign != 0); }
int mz_env_policy_size(const mz_env* e) { return e->e->policySize(); }
int mz_env_feature_size(const mz_env* e) { return e->e->featureSize(); }
int mz_env_legal_mask(const mz_env* e, uint8_t* out)
{
    e->e->legalMask(out);
    return MZ_OK;
}
int mz_env_features(const mz_env* e, int rotation, float* out)
{
    if (rotation < 0 || rotation > 7) { mz::setError("rotation %d out of range", rotation); return MZ_ERR_ARG; }
    e->e->features(rotation, out);
    return MZ_OK;
}

int mz_env_action_from_string(const mz_env* e, const char* action_string)
{
    if (!e || !action_string) { mz::setError("mz_env_action_from_string: NULL argument"); return MZ_ERR_ARG; }
    return e->e->actionFromString(action_string);
}

int mz_env_name(const mz_env* e, char* out, int cap)
{
    if (!e) { mz::setError("mz_env_name: NULL environment"); return MZ_ERR_ARG; }
    const std::string s = e->e->name();
    if (out && cap > 0) { snprintf(out, size_t(cap), "%s", s.c_str()); }
    return static_cast<int>(s.size());
}

int mz_env_feature_bits(const mz_env* e, int rotation, uint32_t* out)
{
    if (rotation < 0 || rotation > 7) { mz::setError("rotation %d out of range", rotation); return MZ_ERR_ARG; }
    e->e->featureBits(rotation, out);
    return MZ_OK;
}

int mz_sort_candidates(int device, const float* policy, int n, int* order_out) { return mz::sortCandidatesOnDevice(device, policy, n, order_out); }

int mz_invert_values_device(int device, const float* values, int n, float* out)
{
    if (mz_device_count() < 1) { mz::setError("mz_invert_values_device: no GPU (libmzgpu has no CPU path)"); return MZ_ERR_DEVICE; }
    if (!values || !out || n < 0) { mz::setError("mz_invert_values_device: bad arguments"); return MZ_ERR_ARG; }
    return mz::invertValuesOnDevice(device, values, n, out);
}

int mz_envdev_playout(int device, const char* game, int board_size, float komi, const int* actions, int count, int root_prefix, const int* rots,
                      uint32_t* feat_out, uint8_t* legal_out, int* terminal_out, float* eval_out, int* player_out)
{
    using namespace mz;
    if (!game) { setError("mz_envdev_playout: NULL game"); return MZ_ERR_ARG; }
    if (mz_device_count() < 1) { setError("mz_envdev_playout: no GPU (libmzgpu has no CPU path)"); return MZ_ERR_DEVICE; }
    if (!actions || !rots || count < 0 || root_prefix < 0 || root_prefix > count) { setError("mz_envdev_playout: bad arguments"); return MZ_ERR_ARG; }
    const bool situational = std::string(game) == "go_situational"; // test access to env_go_ko_rule=situational
    EnvOptions o;
    o.game = situational ? "go" : game;
    o.board_size = board_size;
    o.go_komi = komi;
    o.go_ko_rule = situational ? "situational" : "positional";
    std::unique_ptr<GameEnv> env = createGameEnv(o);
    return envdevPlayout(device, env.get(), komi, actions, count, root_prefix, rots, feat_out, legal_out, terminal_out, eval_out, player_out);
}

int mz_envdev_playout_conf(int device, const char* conf, const int* actions, int count, int root_prefix, const int* rots, uint32_t* feat_out,
                           uint8_t* legal_out, int* terminal_out, float* eval_out, int* player_out)
{
    using namespace mz;
    WorkerConfig c;
    if (!conf || !c.loadFromString(conf)) { return MZ_ERR_ARG; }
    if (mz_device_count() < 1) { setError("mz_envdev_playout_conf: no GPU (libmzgpu has no CPU path)"); return MZ_ERR_DEVICE; }
    if (!actions || !rots || count < 0 || root_prefix < 0 || root_prefix > count) { setError("mz_envdev_playout_conf: bad arguments"); return MZ_ERR_ARG; }
    std::unique_ptr<GameEnv> env = createGameEnv(envOptions(c, 1));
    return envdevPlayout(device, env.get(), c.env_go_komi, actions, count, root_prefix, rots, feat_out, legal_out, terminal_out, eval_out, player_out);
}

} // extern "C"

// the body of both playout entries: root = actions[:root_prefix] on the host engine, then one device move per remaining action
static int envdevPlayout(int device, mz::GameEnv* env, float komi, const int* actions, int count, int root_prefix, const int* rots, uint32_t* feat_out,
                         uint8_t* legal_out, int* terminal_out, float* eval_out, int* player_out)
{
    using namespace mz;
    if (!env || !env->hasDeviceTwin()) { setError("mz_envdev_playout: no device twin for this board"); return MZ_ERR_ARG; }
    for (int i = 0; i < root_prefix; ++i) {
        if (!env->act(actions[i], env->turn())) { setError("mz_envdev_playout: illegal root action %d at move %d", actions[i], i); return MZ_ERR_ARG; }
    }
    const int steps = count - root_prefix + 1, A = env->policySize(), md = steps + 1;
    const int* inv[8];
    const int* fwd[8];
    for (int r = 0; r < 8; ++r) { inv[r] = env->rot()->inv[r].data(); fwd[r] = env->rot()->fwd[r].data(); }
    GoDevice gd;
    int rc = gd.init(device, 1, env->boardSize(), komi, A, steps, md, nullptr, inv, fwd, env->zobristKeys(), env->deviceKind(), env->turnKey());
    if (rc) { return rc; }
    env->exportDeviceRoot(gd.hostSnap(0));
    if ((rc = gd.uploadRoots())) { return rc; }
    // a one-game "tree" that is a single chain: node d = the position after d device moves, kept in slot d
    DevBuf<int> d_i;
    if (!d_i.alloc(size_t(1) + 3 * md)) { setError("mz_envdev_playout: allocation failed"); return MZ_ERR_DEVICE; }
    std::vector<int> h(size_t(1) + 3 * md, 0);
    for (int d = 0; d < md; ++d) {
        h[1 + d] = d;                                                                  // path
        h[1 + md + d] = (d >= 1 && root_prefix + d - 1 < count) ? actions[root_prefix + d - 1] : -1; // path_action
        h[1 + 2 * md + d] = d;                                                         // hslot
    }
    PoolView pv{};
    pv.games = 1; pv.cap = md; pv.A = A; pv.max_depth = md;
    pv.path_len = d_i.p; pv.path = d_i.p + 1; pv.path_action = d_i.p + 1 + md; pv.hslot = d_i.p + 1 + 2 * md;
    const int W32 = (env->boardSize() * env->boardSize() + 31) / 32;
    for (int d = 0; d < steps; ++d) {
        h[0] = d + 1;
        MZ_HIP(hipMemcpy(d_i.p, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice));
        RotPack rp{};
        rotPackSet(rp, 0, rots[d] & 7);
        if ((rc = gd.leafAsync(pv, rp, d))) { return rc; }
        if ((rc = gd.readLeaf(feat_out + size_t(d) * env->numInputChannels() * W32, legal_out + size_t(d) * A, terminal_out + d, eval_out + d, player_out + d))) { return rc; }
    }
    return MZ_OK;
}

extern "C" {

int mz_godev_playout(int device, int board_size, float komi, const int* actions, int count, int root_prefix, const int* rots, uint32_t* feat_out,
                     uint8_t* legal_out, int* terminal_out, float* eval_out, int* player_out)
{
    return mz_envdev_playout(device, "go", board_size, komi, actions, count, root_prefix, rots, feat_out, legal_out, terminal_out, eval_out, player_out);
}

} // extern "C"
