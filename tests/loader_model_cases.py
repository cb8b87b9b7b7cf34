"""Records with known content for the learner-side sampler's model (tests/loader_model.py): one seeded, CPU-only case table.  A row is ONE string,
`<sampler configuration>|<what the records are>`; records(name) turns it into record texts, the same on every machine.

What the records are (`key=value` pairs joined by `,`):
  kind=playout   random legal games on the rules models (tests/rule_envs.py), written by write_record(): per move a P tag with random visit counts on 2 to 6
                 legal moves (sometimes two equal counts, sometimes a single entry, sometimes no tag), R[0], and a V tag in MuZero rows; games=K seeded
                 seed, seed + 1, ...; cut=M ends a game after at most M moves; one game gets a partial DLEN, short=k adds a game of k moves (shorter than the
                 unrolling: absorbing steps), swap=1 makes the first game's second action take the first stone over (Hex), swap=corner adds
                 havannah_rules.SWAP_CORNER;
  kind=oracle    the oracle's self-play (OracleGroup), as tests/test_gpu_loader.py makes its records; cycles=N;
  kind=hand      loader_cases.playout games of Go / Othello / TicTacToe (passes=p: Go's single passes) with the same hand-written tags.
`cap` is the number of batches a GPU test may draw at most to meet the positions the row is there for."""
import functools
import re

import numpy as np

import havannah_rules
import rule_envs

PER = ":learner_use_per=true:learner_per_alpha={a}:learner_per_init_beta={b}"
ATARI = ("env_game=atari:nn_type_name=muzero:actor_num_simulation=4:actor_use_dirichlet_noise=false:actor_use_gumbel=true:actor_use_gumbel_noise=true:"
         "actor_gumbel_sample_size=4:actor_mcts_value_rescale=true:atari_init_q=true:actor_resign_threshold=-2:zero_num_parallel_games=3")


GUMBEL = ":actor_use_dirichlet_noise=false:actor_use_gumbel=true:actor_use_gumbel_noise=true:actor_gumbel_sample_size=4"  # (P tags over every legal move, as floats)


def _mz(u):
    return f":nn_type_name=muzero:learner_muzero_unrolling_step={u}"


ROWS = {
    # ---- the four games no oracle plays: boards of at most 64 points and boards that cross a bitboard word
    "gomoku5_mz5": f"env_game=gomoku:env_board_size=5{_mz(5)}:learner_batch_size=48:program_seed=3|kind=playout,games=4,seed=10,short=3,cap=8",
    "gomoku9_mz3": f"env_game=gomoku:env_board_size=9{_mz(3)}:learner_batch_size=64:program_seed=4|kind=playout,games=4,seed=20,cut=40,short=2,cap=8",
    "gomoku9_az": "env_game=gomoku:env_board_size=9:learner_batch_size=64:program_seed=5|kind=playout,games=4,seed=30,cut=50,cap=6",
    "gomoku15_az": "env_game=gomoku:env_board_size=15:learner_batch_size=32:program_seed=6|kind=playout,games=1,seed=40,cut=40,cap=6",
    "gomoku15oo_az": "env_game=gomoku:env_board_size=15:env_gomoku_rule=outer_open:learner_batch_size=32:program_seed=7|kind=playout,games=1,seed=41,cut=40,cap=6",
    "hex5_mz5": f"env_game=hex:env_board_size=5{_mz(5)}:learner_batch_size=48:program_seed=3|kind=playout,games=4,seed=50,swap=1,short=3,cap=8",
    "hex11_mz3": f"env_game=hex:env_board_size=11{_mz(3)}:learner_batch_size=64:program_seed=4|kind=playout,games=3,seed=60,cut=50,swap=1,short=2,cap=8",
    "hex11_az": "env_game=hex:env_board_size=11:learner_batch_size=64:program_seed=5|kind=playout,games=3,seed=70,cut=60,swap=1,cap=6",
    "hex5_az": "env_game=hex:env_board_size=5:learner_batch_size=48:program_seed=6|kind=playout,games=4,seed=80,swap=1,cap=6",
    "nogo5_mz5": f"env_game=nogo:env_board_size=5{_mz(5)}:learner_batch_size=48:program_seed=3|kind=playout,games=4,seed=90,short=3,cap=8",
    "nogo9_mz3": f"env_game=nogo:env_board_size=9{_mz(3)}:learner_batch_size=64:program_seed=4|kind=playout,games=3,seed=100,cut=40,short=2,cap=8",
    "nogo9_az": "env_game=nogo:env_board_size=9:learner_batch_size=64:program_seed=5|kind=playout,games=3,seed=110,cut=45,cap=6",
    "nogo5_az": "env_game=nogo:env_board_size=5:learner_batch_size=48:program_seed=6|kind=playout,games=4,seed=120,cap=6",
    "havannah4_az": "env_game=havannah:env_board_size=4:learner_batch_size=64:program_seed=3|kind=playout,games=3,seed=130,swap=corner,cap=8",
    "havannah6_az": "env_game=havannah:env_board_size=6:learner_batch_size=64:program_seed=4|kind=playout,games=3,seed=140,cut=60,cap=6",
    # ---- the games the oracle plays: its self-play records, and hand-written tags over random games with passes
    "go9_az": f"env_game=go:env_board_size=9:actor_num_simulation=8:zero_num_parallel_games=4{GUMBEL}:learner_batch_size=64:program_seed=13|kind=oracle,cycles=1575,cap=3",
    "go9_mz5": f"env_game=go:env_board_size=9:actor_num_simulation=8:zero_num_parallel_games=3{GUMBEL}{_mz(5)}:learner_batch_size=64:program_seed=21|kind=oracle,cycles=1575,cap=6",
    "othello8_az": f"env_game=othello:env_board_size=8:actor_num_simulation=8:zero_num_parallel_games=4{GUMBEL}:learner_batch_size=64:program_seed=4|kind=oracle,cycles=630,cap=3",
    "tictactoe_mz3": f"env_game=tictactoe:actor_num_simulation=8:zero_num_parallel_games=8{_mz(3)}:learner_batch_size=64:program_seed=9|kind=oracle,cycles=360,cap=3",
    "go9_hand_mz3": f"env_game=go:env_board_size=9{_mz(3)}:learner_batch_size=64:program_seed=5|kind=hand,games=3,seed=150,cut=50,passes=0.1,short=2,cap=6",
    "go5_hand_az": "env_game=go:env_board_size=5:learner_batch_size=48:program_seed=6|kind=hand,games=3,seed=160,cut=30,passes=0.15,cap=6",
    # beyond two 64-bit words per plane, the records played by the rules model (tests/go_rules.py) and not by the oracle: captures, passes, two passes at the end
    "go13_hand_az": "env_game=go:env_board_size=13:learner_batch_size=32:program_seed=7|kind=hand,by=model,games=2,seed=200,cut=120,passes=0.05,cap=6",
    "go19_hand_mz3": f"env_game=go:env_board_size=19{_mz(3)}:learner_batch_size=32:program_seed=8|kind=hand,by=model,games=2,seed=210,cut=150,passes=0.05,short=2,cap=6",
    "othello8_hand_mz3": f"env_game=othello:env_board_size=8{_mz(3)}:learner_batch_size=64:program_seed=7|kind=hand,games=2,seed=170,short=2,cap=6",
    "othello4_hand_az": "env_game=othello:env_board_size=4:learner_batch_size=32:program_seed=8|kind=hand,games=4,seed=180,cap=6",
    "tictactoe_hand_az": "env_game=tictactoe:learner_batch_size=32:program_seed=9|kind=hand,games=5,seed=190,cap=6",
    # ---- Atari-shaped games: n-step values, life loss, intermediate sequences, prioritised replay (loaded from a file: the path that computes the sum)
    "atari_n3": (f"{ATARI}:actor_mcts_reward_discount=0.997:zero_actor_intermediate_sequence_length=10:learner_n_step_return=3:learner_muzero_unrolling_step=2:"
                 f"env_atari_episode_length=45:learner_batch_size=24:program_seed=5{PER.format(a=0.5, b=0.4)}|kind=oracle,cycles=250,cap=10"),
    "atari_n5": (f"{ATARI}:actor_mcts_reward_discount=0.9:zero_actor_intermediate_sequence_length=12:learner_n_step_return=5:learner_muzero_unrolling_step=3:"
                 f"env_atari_episode_length=40:learner_batch_size=24:program_seed=6{PER.format(a=1.0, b=1.0)}|kind=oracle,cycles=230,cap=10"),
    "atari_n1_short": (f"{ATARI}:actor_mcts_reward_discount=0.997:zero_actor_intermediate_sequence_length=0:learner_n_step_return=1:learner_muzero_unrolling_step=2:"
                       f"env_atari_episode_length=6:learner_batch_size=16:program_seed=7{PER.format(a=1.0, b=0.4)}|kind=oracle,cycles=70,cap=10"),
}
NEW_GAMES = [n for n, r in ROWS.items() if "kind=playout" in r]
ORACLE_GAMES = [n for n in ROWS if n not in NEW_GAMES]
ATARI_ROWS = [n for n in ROWS if n.startswith("atari")]
PER_ROWS = [n for n, r in ROWS.items() if "learner_use_per=true" in r]
ROTATED_NEW = [n for n in NEW_GAMES if n.startswith(("gomoku", "nogo"))]
# the two rows whose sampling frequencies are tested (uniform, prioritised)
FREQUENCY_ROWS = ("go9_az", "atari_n5")

DESCS = {"go": ("go_9x9", 18, 9, 9, 8, 9, 9, 1, 1, 82, 16, 1), "othello": ("othello_8x8", 4, 8, 8, 8, 8, 8, 1, 1, 65, 16, 1),
         "tictactoe": ("tictactoe", 4, 3, 3, 16, 3, 3, 1, 2, 9, 256, 1), "atari": ("atari_ms_pacman", 32, 96, 96, 32, 6, 6, 18, 1, 18, 32, 601)}


def conf_of(name):
    return ROWS[name].split("|")[0]


def spec_of(name):
    return dict(x.split("=") for x in ROWS[name].split("|")[1].split(","))


def _kv(conf):
    return dict(x.split("=", 1) for x in conf.split(":") if x)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def p_tag(rng, legal, played):
    """a P tag over 2 to 6 legal moves (the played one among them), or a single entry, or none ('')"""
    u = rng.random()
    if u < 0.15:
        return ""
    others = [int(a) for a in legal if a != played]
    k = 0 if u < 0.3 else min(len(others), int(rng.integers(1, 6)))
    acts = [played] + [int(a) for a in rng.choice(others, k, replace=False)] if k else [played]
    counts = [int(c) for c in rng.integers(1, 40, len(acts))]
    if len(acts) >= 2 and rng.random() < 0.3:
        counts[1] = counts[0]  # a tie
    order = rng.permutation(len(acts))
    return ",".join(f"{acts[i]}:{counts[i]}" for i in order)


def write_record(gm, sz, result, moves, dlen=None, muzero=False, rng=None):
    """moves = [(action, P text)]; colours alternate from B; R[0] always, V[...] (6 decimals, as std::to_string writes) in MuZero rows"""
    s = f"(;GM[{gm}]RE[{result}]SZ[{sz}]" + (f"DLEN[{dlen[0]}-{dlen[1]}]" if dlen else "")
    for i, (a, p) in enumerate(moves):
        s += f";{'BW'[i & 1]}[{a}]" + (f"P[{p}]" if p else "") + (f"V[{rng.uniform(-1, 1):.6f}]" if muzero else "") + "R[0]"
    return s + ")"


def _result(score, rng):
    return int(score) if score else int(rng.choice([-1, 1]))  # (a game that was cut short: as if one side resigned)


def _partial(length, rng):
    """a data range that leaves out the start and, mostly, the end of a game of more than 4 moves"""
    return int(rng.integers(1, length // 3 + 1)), int(rng.integers(2 * length // 3, length))


def playout_records(conf, spec):
    game, n, _ = rule_envs.parse(conf)
    muzero = "nn_type_name=muzero" in conf
    gm = {"gomoku": f"gomoku_{'oo_' if 'outer_open' in conf else ''}{n}x{n}", "hex": f"hex_{n}x{n}", "nogo": f"nogo_{n}x{n}", "havannah": f"havannah{n}x{n}"}[game]
    out = []
    lengths = [int(spec["cut"]) if "cut" in spec else None] * int(spec["games"]) + ([int(spec["short"])] if "short" in spec else [])
    for k, cut in enumerate(lengths):
        rng = np.random.default_rng(int(spec["seed"]) + k)
        env = rule_envs.RuleEnv(conf)
        moves = []
        while not env.terminal() and (cut is None or len(moves) < cut):
            legal = np.nonzero(env.legal())[0]
            a = moves[0][0] if (spec.get("swap") == "1" and k == 0 and len(moves) == 1) else int(rng.choice(legal))
            board = [x for x in legal if not (len(moves) == 1 and game in ("hex", "havannah") and x == moves[0][0])]  # (the swap is no ordinary candidate)
            moves.append((a, p_tag(rng, board if a in board else list(board) + [a], a)))
            env.act(a, env.turn())
        dlen = _partial(len(moves), rng) if k == 1 % len(lengths) and len(moves) > 4 else None
        out.append(write_record(gm, n, _result(env.score(), rng), moves, dlen, muzero, rng))
    if spec.get("swap") == "corner":
        m = havannah_rules.Havannah(n)
        acts = [m.ident(c) for c in havannah_rules.SWAP_CORNER["actions"]]
        assert n == havannah_rules.SWAP_CORNER["N"]
        out.insert(0, write_record(gm, n, -1, [(a, "") for a in acts]))
    return out


def model_go_records(conf, spec):
    """hand-written tags over games the Go rules model plays: uniformly random legal points, a pass with probability `passes`, two passes after `cut` moves (more than 4)"""
    game, n, _ = rule_envs.parse(conf)
    muzero = "nn_type_name=muzero" in conf
    out = []
    lengths = [int(spec["cut"])] * int(spec["games"]) + ([int(spec["short"])] if "short" in spec else [])
    for k, cut in enumerate(lengths):
        rng = np.random.default_rng(int(spec["seed"]) + k)
        env = rule_envs.RuleEnv(conf)
        moves = []
        while not env.terminal() and not (cut <= 4 and len(moves) >= cut):  # (a short game is cut off, as if one side resigned)
            legal = np.nonzero(env.legal())[0]
            a = n * n if len(moves) >= cut or len(legal) == 1 or rng.random() < float(spec["passes"]) else int(rng.choice(legal[:-1]))
            moves.append((a, p_tag(rng, legal, a)))
            env.act(a, env.turn())
        dlen = _partial(len(moves), rng) if k == 1 % len(lengths) and len(moves) > 4 else None
        out.append(write_record(game, n, _result(env.score(), rng), moves, dlen, muzero, rng))
    return out


def hand_records(conf, spec):
    if spec.get("by") == "model":
        return model_go_records(conf, spec)
    import loader_cases as lc
    import oracle_lib
    kv = _kv(conf)
    game, n = kv["env_game"], int(kv.get("env_board_size", 3))
    muzero = "nn_type_name=muzero" in conf
    out = []
    lengths = [int(spec["cut"]) if "cut" in spec else None] * int(spec["games"]) + ([int(spec["short"])] if "short" in spec else [])
    for k, cut in enumerate(lengths):
        seed = int(spec["seed"]) + k
        rng = np.random.default_rng(seed)
        acts = lc.playout(n, seed, max_moves=cut, pass_prob=float(spec.get("passes", 0)), game=game, end_with_passes=game == "go" and cut is not None and cut > 4)
        env = oracle_lib.OracleEnv(lc.game_conf(game, n))
        moves = []
        for a in acts:
            moves.append((a, p_tag(rng, np.nonzero(env.legal_mask())[0], a)))
            assert env.act(a)
        dlen = _partial(len(moves), rng) if k == 1 % len(lengths) and len(moves) > 4 else None
        out.append(write_record(game, n, _result(env.eval_score() if env.is_terminal() else 0, rng), moves, dlen, muzero, rng))
    return out


def oracle_lines(conf, spec):
    """`SelfPlay ... #` lines of the oracle's self-play side (tests/test_gpu_loader.py _records)"""
    import oracle_lib
    kv = _kv(conf)
    game = kv["env_game"]
    dargs = DESCS[game]
    typ = "muzero_atari" if game == "atari" else kv.get("nn_type_name", "alphazero")
    od = oracle_lib.make_desc(*dargs[:10], vh=dargs[10], dv=dargs[11], type_name=typ)
    actor = ":".join(f"{k}={v}" for k, v in kv.items() if not k.startswith("learner_use_per") and not k.startswith("learner_per") and k not in ("learner_batch_size", "program_seed"))
    og = oracle_lib.OracleGroup(actor + ":program_seed=7:nn_file_name=weight_iter_5.pt:zero_num_threads=1", od, oracle_lib.gen_weights(od, 2))
    og.cycles(int(spec["cycles"]))
    return og.lines()


def bare(line):
    """the record inside a `SelfPlay ... #` line (zero_server.cpp writes the bare records to the sgf file)"""
    return line.split(" ", 5)[5][:-2] if line.startswith("SelfPlay") else line


@functools.lru_cache(None)
def records(name):
    conf, spec = conf_of(name), spec_of(name)
    recs = {"playout": playout_records, "hand": hand_records, "oracle": lambda c, s: [bare(l) for l in oracle_lines(c, s)]}[spec["kind"]](conf, spec)
    assert recs, name
    return tuple(recs)


def cap(name):
    return int(spec_of(name)["cap"])


P_TAG = re.compile(r"P\[([^\]]*)\]")


def p_tag_kinds(recs):
    """(a tag with two equal counts exists, a single-entry tag exists, a move without a tag exists)"""
    tags = [t for r in recs for t in P_TAG.findall(r)]
    counts = [[x.split(":")[1] for x in t.split(",")] for t in tags]
    moves = sum(len(re.findall(r";[BW]\[", r)) for r in recs)
    return any(len(set(c)) < len(c) for c in counts), any(len(c) == 1 for c in counts), moves > len(tags)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# what the CPU and the GPU test share
# ---------------------------------------------------------------------------------------------------------------------------------------------------
PLANES = {"go": 18, "nogo": 18, "othello": 4, "tictactoe": 4, "gomoku": 4, "hex": 4, "havannah": 20}
NAMES = ["features", "action_features", "policy", "value", "reward", "loss_scale", "sampled_index"]


def buffers(cfg):
    """the seven arrays of one batch, in sample_data's order, for a loader_model.Cfg"""
    nf = 32 * 96 * 96 if cfg.game == "atari" else PLANES[cfg.game] * cfg.points
    U, B = cfg.unroll, cfg.batch
    sizes = (nf, U * cfg.action_size, (U + 1) * cfg.policy_size, (U + 1) * cfg.value_size, U * cfg.value_size)
    return [np.zeros((B, max(k, 1)), np.float32) for k in sizes] + [np.zeros(B, np.float32), np.zeros((B, 2), np.int32)]


def write_file(path, recs):
    with open(path, "w") as f:
        f.write("\n".join(recs) + "\n")
    return path


def fixed_values(cfg, salt=0):
    """the values a trainer might hand to update_priority: [unroll + 1][batch] on the transformed scale, none of them a 6-decimal number after the inversion"""
    return (np.linspace(-2.0, 3.0, (cfg.unroll + 1) * cfg.batch) + 0.0137 * salt).astype(np.float32).reshape(cfg.unroll + 1, cfg.batch)


def chi_square(model, counts):
    """(statistic, degrees of freedom, bound) of the drawn (game, position) counts against priority / sum over the data ranges; bound = dof + 5 * sqrt(2 * dof)"""
    total = sum(counts.values())
    stat, cells = 0.0, 0
    for g in range(model.num_games()):
        a, b = model.data_range(g)
        for pos in range(a, b + 1):
            expected = total * float(model.probability(g, pos))
            assert expected >= 20, f"(game {g}, position {pos}): expected count {expected:.1f} < 20, draw more batches"
            stat += (counts.get((g, pos), 0) - expected) ** 2 / expected
            cells += 1
    assert set(counts) <= {(g, p) for g in range(model.num_games()) for p in range(model.data_range(g)[0], model.data_range(g)[1] + 1)}, "a draw outside the data range"
    dof = cells - 1
    return stat, dof, dof + 5 * (2 * dof) ** 0.5


def batches_for_frequencies(model):
    """the number of batches after which every position's expected count is at least 20 (and a fifth more)"""
    least = min(float(model.probability(g, p)) for g in range(model.num_games()) for p in range(model.data_range(g)[0], model.data_range(g)[1] + 1))
    return int(np.ceil(24 / least / model.cfg.batch))
