// TEST INFRASTRUCTURE ONLY.  The HOST half of match play (mz_worker_create_match: the schedule, the colour rule, serial numbers and fillers, the tally, the
// `Match` lines) under ThreadSanitizer / AddressSanitizer + UBSan on a machine without a GPU: this file + the product's host sources + fake_device.cpp (the
// oracle behind the device seam), built by tests/test_match_sanitizers.py with the flags tests/csrc/Makefile uses for host_check.
//
//   match_check "<conf>" <game_name> cin h w ch hh hw ac blocks actions vh dv type seed_a seed_b
//       plays the match of the configuration (mz_match_games, zero_num_parallel_games; lock-step with the rules on the host: mz_device_env=false) to its end
//       and prints every `Match` line (L), every slot's record afterwards (R) and the tally (S).  Checked in the program: the tally again from the lines;
//       run_cycles returns 0 after the end; and with seed_a == seed_b (A = B) the moves of every game are those of a plain worker created from the same
//       configuration and weights in the same program.  Exit status 0: all of it held.
#include "../../include/mzgpu.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
long mzo_net_param_count(const mz_net_desc* d);
void mzo_net_generate(const mz_net_desc* d, unsigned long long seed, float* out);
}

static int fail(const char* what) { fprintf(stderr, "match_check: %s: %s\n", what, mz_last_error()); return 1; }

static bool popLines(mz_worker* wk, std::vector<std::string>* out)
{
    if (mz_worker_wait_lines(wk) < 0) { return false; }
    std::vector<char> buf(1 << 16);
    for (;;) {
        const int need = mz_worker_pop_line(wk, nullptr, 0);
        if (need == 0) { return true; }
        if (need < 0) { return false; }
        if (static_cast<size_t>(need) >= buf.size()) { buf.resize(static_cast<size_t>(need) + 1); }
        if (mz_worker_pop_line(wk, buf.data(), static_cast<int>(buf.size())) < 0) { return false; }
        out->push_back(buf.data());
    }
}

// the moves of a line: everything behind the root's tags
static std::string movesOf(const std::string& line)
{
    const size_t root = line.find("(;");
    const size_t first = root == std::string::npos ? std::string::npos : line.find(';', root + 2);
    return first == std::string::npos ? std::string() : line.substr(first);
}

static std::string tagOf(const std::string& line, const char* key)
{
    const std::string k = std::string(key) + "[";
    const size_t at = line.find(k);
    if (at == std::string::npos) { return ""; }
    return line.substr(at + k.size(), line.find(']', at) - at - k.size());
}

int main(int argc, char** argv)
{
    if (argc != 17) { fprintf(stderr, "usage: see the header comment\n"); return 2; }
    const std::string conf = argv[1];
    mz_net_desc d;
    memset(&d, 0, sizeof(d));
    snprintf(d.game_name, sizeof(d.game_name), "%s", argv[2]);
    int* fields[] = {&d.num_input_channels, &d.input_channel_height, &d.input_channel_width, &d.num_hidden_channels, &d.hidden_channel_height, &d.hidden_channel_width,
                     &d.num_action_feature_channels, &d.num_blocks, &d.action_size, &d.num_value_hidden_channels, &d.discrete_value_size, &d.type};
    for (int i = 0; i < 12; ++i) { *fields[i] = atoi(argv[3 + i]); }
    const unsigned long long seed_a = strtoull(argv[15], nullptr, 10), seed_b = strtoull(argv[16], nullptr, 10);
    std::vector<float> wa(static_cast<size_t>(mzo_net_param_count(&d))), wb(wa.size());
    mzo_net_generate(&d, seed_a, wa.data());
    mzo_net_generate(&d, seed_b, wb.data());

    mz_worker* wk = mz_worker_create_match(0, conf.c_str(), &d, wa.data(), wa.size(), wb.data(), wb.size());
    if (!wk) { return fail("mz_worker_create_match"); }
    if (mz_worker_lanes(wk) != 2) { fprintf(stderr, "match_check: %d lanes\n", mz_worker_lanes(wk)); return 1; }
    if (mz_worker_command(wk, "start") < 0) { return fail("start"); }
    if (mz_worker_command(wk, "load_model x.pt") != MZ_ERR_STATE || mz_worker_set_weights(wk, wa.data(), wa.size()) != MZ_ERR_STATE) {
        fprintf(stderr, "match_check: a running match took new weights\n");
        return 1;
    }
    const int cpm = mz_worker_cycles_per_move(wk);
    mz_match_stats st;
    std::vector<std::string> lines;
    for (int guard = 0;; ++guard) {
        if (mz_worker_match_stats(wk, &st) != MZ_OK) { return fail("match_stats"); }
        if (st.done) { break; }
        if (guard > 10000) { fprintf(stderr, "match_check: the match does not end\n"); return 1; }
        if (mz_worker_run_cycles(wk, cpm) < 0) { return fail("run_cycles"); }
        if (!popLines(wk, &lines)) { return fail("pop_line"); }
    }
    if (mz_worker_run_cycles(wk, cpm) != 0 || mz_worker_run_cycles(wk, 1) != 0) { fprintf(stderr, "match_check: a finished match ran further cycles\n"); return 1; }
    for (const std::string& l : lines) { printf("L %s\n", l.c_str()); }
    const char* g = strstr(conf.c_str(), "zero_num_parallel_games=");
    const int games = g ? atoi(g + strlen("zero_num_parallel_games=")) : 0;
    std::vector<char> buf(1 << 16);
    for (int i = 0; i < games; ++i) {
        if (mz_worker_peek_record(wk, i, buf.data(), static_cast<int>(buf.size())) < 0) { return fail("peek_record"); }
        printf("R %s\n", buf.data());
    }
    printf("S games_started=%llu games_finished=%llu moves=%llu filler_games=%llu a_first=%llu,%llu,%llu a_second=%llu,%llu,%llu resignations=%llu steps=%llu done=%d\n",
           (unsigned long long)st.games_started, (unsigned long long)st.games_finished, (unsigned long long)st.moves, (unsigned long long)st.filler_games,
           (unsigned long long)st.a_first[0], (unsigned long long)st.a_first[1], (unsigned long long)st.a_first[2], (unsigned long long)st.a_second[0],
           (unsigned long long)st.a_second[1], (unsigned long long)st.a_second[2], (unsigned long long)st.resignations, (unsigned long long)st.steps, st.done);
    mz_worker_destroy(wk);

    // the tally again, from the lines alone
    unsigned long long first[3] = {0, 0, 0}, second[3] = {0, 0, 0};
    for (const std::string& l : lines) {
        if (l.compare(0, 6, "Match ") != 0) { fprintf(stderr, "match_check: not a Match line: %.60s\n", l.c_str()); return 1; }
        char word[16], flag[16];
        int dlen = 0, length = 0;
        float score = 0;
        if (sscanf(l.c_str(), "%15s %15s %d %d %f", word, flag, &dlen, &length, &score) != 5) { fprintf(stderr, "match_check: unreadable line head\n"); return 1; }
        const int idx = score > 0 ? 0 : (score < 0 ? 2 : 1);
        const std::string pb = tagOf(l, "PB"), pw = tagOf(l, "PW");
        if (!((pb == "A" && pw == "B") || (pb == "B" && pw == "A"))) { fprintf(stderr, "match_check: PB[%s]PW[%s]\n", pb.c_str(), pw.c_str()); return 1; }
        if (pb == "A") { ++first[idx]; } else { ++second[2 - idx]; }
    }
    if (lines.size() != st.games_finished || memcmp(first, st.a_first, sizeof(first)) != 0 || memcmp(second, st.a_second, sizeof(second)) != 0) {
        fprintf(stderr, "match_check: the tally of the lines (%llu,%llu,%llu | %llu,%llu,%llu over %zu lines) is not mz_match_stats'\n", first[0], first[1], first[2], second[0],
                second[1], second[2], lines.size());
        return 1;
    }

    if (seed_a == seed_b) { // A = B: a plain worker's games, move for move
        mz_worker* plain = mz_worker_create(0, conf.c_str(), &d, wa.data(), wa.size());
        if (!plain) { return fail("mz_worker_create"); }
        if (mz_worker_command(plain, "start") < 0) { return fail("start"); }
        std::vector<std::string> pl;
        for (int guard = 0; pl.empty(); ++guard) {
            if (guard > 10000) { fprintf(stderr, "match_check: the plain worker finishes no game\n"); return 1; }
            if (mz_worker_run_cycles(plain, cpm) < 0) { return fail("run_cycles"); }
            if (!popLines(plain, &pl)) { return fail("pop_line"); }
        }
        mz_worker_destroy(plain);
        if (pl[0].compare(0, 9, "SelfPlay ") != 0) { fprintf(stderr, "match_check: the plain worker printed %.60s\n", pl[0].c_str()); return 1; }
        for (const std::string& l : lines) {
            if (movesOf(l).empty() || movesOf(l) != movesOf(pl[0])) {
                fprintf(stderr, "match_check: A = B, but a game differs from the plain worker's:\n  %s\n  %s\n", l.c_str(), pl[0].c_str());
                return 1;
            }
        }
        printf("P %s\n", pl[0].c_str());
    }
    return 0;
}
