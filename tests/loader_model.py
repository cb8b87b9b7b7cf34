"""A plain, slow model of the reference's learner-side sampler, written from the reference's text: what one sampled (game, position) of a batch holds, from
the configuration string and the record text alone.  This file imports neither the oracle nor the product.  Every float of the reference is a numpy float32
here and every promotion to double is spelled out; only the pow()-based quantities (priorities, loss scale) are kept in float64 and compared with a bound.

The rules, with the reference's lines:

- record text (environment/base/base_env.h:150-205): a state machine over `(;KEY[value]...;B[a]KEY[value]...)`; `\\` escapes the next character of a value;
  a key after `;` is a move (its first letter the player, the value a number), keys before the first move are the game's tags (GM, SZ, RE, SD, DLEN, OBS,
  ...), keys after a move are that move's (P, V, R, L); a record counts only if its `)` was met.  Text before the `(` is skipped: a `SelfPlay ... #` line
  of a worker parses like the bare record.  Havannah's SZ is the edge size N, its array is (2N - 1) x (2N - 1);
- data range (base_env.h:268-276): DLEN[a-b] when present, else 0 .. max(0, moves - 1);
- policy (base_env.h:243-266): the P tag's `action:count` pairs in the record's order, each count std::stof, written to the ROTATED action, the total a
  float32 sum in that order, then every entry divided by the total in float32; no P tag: 1 on the rotated move; past the end: 1.0f / size everywhere;
- rotation (utils/rotation.h:53-92): getPositionByRotating, the pass kept.  Go, NoGo, Othello, TicTacToe and Gomoku rotate (go.h:140-141, nogo.h:88-91,
  othello.h:82-83, tictactoe.h:50-51, gomoku.h:62-63); Hex, Havannah and Atari ignore the rotation (hex.h:78-79, havannah.h:168-169, atari.h:121-122).  The planes go through
  the REVERSED rotation inside the engines' getFeatures (the rules models do that);
- value: board games RE (getReturn, go.h:137, othello.h:79, tictactoe.h:47, gomoku.h:59, hex.h:75, havannah.h:165 — the same float for either player);
  Atari (atari.h:115, atari.cpp:259-293): toDiscreteValue(transformValue(calculateNStepValue)) inside the game, toDiscreteValue(0) past it;
  calculateNStepValue: bootstrap = pow(discount, n) [double] * V[pos + n] [float] stored as float, 0 when pos + n is past the end or that move has an L tag;
  then for index = pos .. min(pos + n, moves) - 1: an L tag with lives > 0 RETURNS what has been summed (without the bootstrap), else
  value = float(double(value) + pow(discount, index - pos) [double] * R[index]); last value += bootstrap in float;
- transformValue / invertValue (utils/utils.h:93-108): tests/test_value_transform.py's closed forms;
- toDiscreteValue (atari.cpp:279-293): 601 bins, shift 300, floor and ceil clamped to the range; equal: 1 there; else bin floor = float(ceil) - value and
  bin ceil = value - float(floor), both float32;
- reward (base_env.h:279, atari.h:116): std::stof of R inside the game (Atari: transformed and split into bins), 0 past the end (Atari: bin 300);
- action features: Go / NoGo / Othello (go.cpp:725-737, othello.cpp:264-275): the rotated point, a pass leaves the plane empty; past the end a draw
  d = randInt() % (P + 1) that is set only when d < moves; TicTacToe, Gomoku (rotated) and Hex (not rotated) (tictactoe.cpp:148-155, gomoku.cpp:177-184,
  hex.cpp:364-371): the point, past the end a random point; Atari (atari.cpp:223-235): plane `action` of 18 x 6 x 6 all ones, past the end a random plane;
  Havannah's throws (havannah.cpp:498-501): no MuZero.  check_absorbing_plane() states what any draw satisfies;
- planes: Gomoku, Hex, NoGo, Havannah by replaying the first min(position, moves) moves (base_env.h:235-241) on tests/*_rules.py, once per game, and
  permuting the cached planes for a rotation; Atari (atari.cpp:199-221,237-249): the OBS tag is gzip as hex (utils/utils.h:66-91) of 3 x 96 x 96 byte
  screens, the LAST ones of the game: observations[moves] is the last screen; 8 history steps i = pos - 7 .. pos of [float(action[i - 1]) / 18 (0 before the
  first move), R, G, B / 255.0f], zeros for i < 0; a missing screen replays the whole position from the SD seed (tests/atari_synth.py);
- priorities (learner/data_loader.cpp:24-51): position priority = pow(PER ? getPriority : 1, alpha) for the data range, 0 before it; the game's priority is
  their float sum; getPriority is 1 for board games (base_env.h:286) and float(fabs(n-step - V[pos]) + 1e-6) for Atari (atari.h:117);
- loss scale (data_loader.cpp:66-74): 1 without PER, else pow(num_data * priority / sum, -beta), the sum being the one loadDataFromFile (216-224) or
  updatePriority last computed (0 before either: the scale is then pow(inf, -beta) = 0);
- updatePriority (data_loader.cpp:233-253): per sample in batch order, for step 0 .. unroll: V[pos + step] = std::to_string(invertValue(values[step][b]))
  — the "%f" text, 6 decimals — where pos + step is inside the game; then the sample's priority is recomputed from the text; at last every game's sum and
  the grand sum.

`wrong` names one deliberately wrong reading (WRONG); tests/test_loader_model.py shows that the case table tells each from the model."""
import gzip
import math
import re
from fractions import Fraction
from functools import lru_cache

import numpy as np

import rule_envs
from atari_synth import AtariSynth
from gomoku_rules import REVERSED, rotate_pos
from test_value_transform import closed_form_invert, closed_form_transform

f32 = np.float32
f64 = np.float64
ROTATING = ("go", "nogo", "othello", "tictactoe", "gomoku")
WITH_PASS = ("go", "nogo", "othello")
RULES = rule_envs.GAMES
BINS, RES, HIST, ATARI_ACTIONS, HIDDEN = 601, 96, 8, 18, 36
WRONG = ("policy_inverse_rotation", "policy_not_rotated", "action_not_rotated", "counts_not_permuted", "nstep_off_by_one", "l_cut_ignored",
         "bootstrap_at_l", "screens_from_start", "value_of_mover", "priority_without_text")


@lru_cache(None)
def stof(text):
    """std::stof: the float32 nearest to the decimal text (ties to even), without a detour through double rounding"""
    d = float(text)
    f = f32(d)
    if float(f) == d or not np.isfinite(f):
        return f
    exact = Fraction(text)
    best = min((f, np.nextafter(f, f32(-np.inf)), np.nextafter(f, f32(np.inf))),
               key=lambda c: (abs(Fraction(float(c)) - exact), int(c.view(np.uint32)) & 1))
    return f32(best)


def to_string(x):
    """std::to_string(float): printf("%f") of the value as a double"""
    return "%f" % float(f32(x))


class Cfg:
    """the keys of config/configuration.cpp the sampler reads, from a `key=value:...` string, with the reference's defaults"""

    def __init__(self, conf):
        kv = dict(x.split("=", 1) for x in conf.split(":") if x)
        self.game = kv["env_game"]
        self.n = int(kv.get("env_board_size", 0)) or {"tictactoe": 3, "go": 9, "othello": 8, "atari": 0, **rule_envs.DEFAULT_BOARD}[self.game]
        self.muzero = kv.get("nn_type_name", "alphazero") == "muzero"
        self.unroll = int(kv.get("learner_muzero_unrolling_step", 5)) if self.muzero else 0
        self.n_step = int(kv.get("learner_n_step_return", 10 if self.game == "atari" else 0))
        self.discount = f32(kv.get("actor_mcts_reward_discount", 1.0))
        self.per = kv.get("learner_use_per", "false").lower() in ("true", "1")
        self.alpha = f32(kv.get("learner_per_alpha", 1.0))
        self.beta = f32(kv.get("learner_per_init_beta", 1.0))
        self.batch = int(kv.get("learner_batch_size", 1024))
        self.episode_length = int(kv.get("env_atari_episode_length", 0))
        self.conf = conf
        side = 2 * self.n - 1 if self.game == "havannah" else self.n
        self.points = side * side
        self.policy_size = ATARI_ACTIONS if self.game == "atari" else self.points + (self.game in WITH_PASS)
        self.action_size = ATARI_ACTIONS * HIDDEN if self.game == "atari" else self.points
        self.rotations = tuple(range(8)) if self.game in ROTATING else (0,)
        self.value_size = BINS if self.game == "atari" else 1


class Record:
    """one record's tags and moves (base_env.h:150-205); ok = the closing parenthesis was met"""

    def __init__(self, text):
        self.tags, self.moves = {}, []  # moves: [player letter, action, {tag: value}]
        key, value, state, accept, escape = "", "", "(", False, False
        for c in text:
            if state == "(":
                if not accept:
                    accept = c == "("
                else:
                    state, accept = (";" if c == ";" else "x"), False
            elif state == ";":
                if c == ";":
                    accept = True
                elif c in "[)":
                    state = c
                elif c.isprintable() and not c.isspace():
                    key += c
            elif state == "[":
                if c == "\\" and not escape:
                    escape = True
                elif c != "]" or escape:
                    value += c
                    escape = False
                else:
                    if accept:
                        assert value[:1].isdigit(), f"a move that is no number: {value!r}"
                        self.moves.append([key[0], int(re.match(r"\d+", value).group()), {}])
                        accept = False
                    elif self.moves:
                        self.moves[-1][2][key] = value
                    else:
                        self.tags[key] = value
                    key, value, state = "", "", ";"
        self.ok = state == ")"
        self.actions = [m[1] for m in self.moves]

    def __len__(self): return len(self.moves)

    def data_range(self):
        dlen = self.tags.get("DLEN", "")
        if not dlen:
            return 0, max(0, len(self.moves) - 1)
        return int(re.match(r"\s*[-+]?\d+", dlen).group()), int(re.match(r"\s*[-+]?\d+", dlen[dlen.find("-") + 1:]).group())

    def info(self, pos, tag): return self.moves[pos][2].get(tag, "")


class LoaderModel:
    def __init__(self, conf, wrong=None):
        assert wrong is None or wrong in WRONG, wrong
        self.cfg, self.wrong = Cfg(conf), wrong
        self.records, self.prio, self.game_prio, self.sum = [], [], [], f64(0)
        self._planes, self._screens = {}, {}

    # ---- loading -------------------------------------------------------------------------------------------------------------------------------------
    def add(self, text):
        rec = Record(text)
        if not rec.ok:
            return False
        if "SZ" in rec.tags and self.cfg.game != "atari":
            assert int(rec.tags["SZ"]) == self.cfg.n, (rec.tags["SZ"], self.cfg.n)
        self.records.append(rec)
        g = len(self.records) - 1
        first, last = rec.data_range()
        self.prio.append([f64(0)] * (last + 1))
        for pos in range(first, last + 1):
            self.prio[g][pos] = self.position_priority(g, pos)
        self.game_prio.append(sum(self.prio[g], f64(0)))
        return True

    def finish(self):
        """what loadDataFromFile does after the last record: the grand sum"""
        self.sum = sum(self.game_prio, f64(0))

    def load(self, texts):
        for t in texts:
            assert self.add(t), t[:80]
        self.finish()
        return self

    def num_games(self): return len(self.records)
    def num_data(self): return sum(b - a + 1 for a, b in (r.data_range() for r in self.records))
    def data_range(self, g): return self.records[g].data_range()

    # ---- rotation ------------------------------------------------------------------------------------------------------------------------------------
    def rotate_action(self, a, rot):
        if self.cfg.game not in ROTATING or a == self.cfg.points:
            return a
        return rotate_pos(rot, a, self.cfg.n)

    # ---- targets -------------------------------------------------------------------------------------------------------------------------------------
    def policy(self, g, pos, rot):
        rec, A = self.records[g], self.cfg.policy_size
        out = np.zeros(A, np.float32)
        if pos >= len(rec):
            out[:] = f32(1) / f32(A)
            return out
        prot = {"policy_inverse_rotation": REVERSED[rot], "policy_not_rotated": 0}.get(self.wrong, rot)
        text = rec.info(pos, "P")
        if not text:
            out[self.rotate_action(rec.actions[pos], prot)] = 1
            return out
        total = f32(0)
        for item in text.split(","):
            a, count = int(item[:item.find(":")]), stof(item[item.find(":") + 1:])
            out[a if self.wrong == "counts_not_permuted" else self.rotate_action(a, prot)] = count
            total = f32(total + count)
        return out / total  # float32 / float32

    def value(self, g, pos):
        rec = self.records[g]
        if self.cfg.game != "atari":
            v = stof(rec.tags["RE"])
            if self.wrong == "value_of_mover" and pos < len(rec) and rec.moves[pos][0] == "W":
                v = f32(-v)
            return np.array([v], np.float32)
        return discrete(closed_form_transform(self.n_step_value(g, pos)) if pos < len(rec) else f32(0))

    def reward(self, g, pos):
        rec = self.records[g]
        r = stof(rec.info(pos, "R")) if pos < len(rec) else f32(0)
        if self.cfg.game != "atari":
            return np.array([r], np.float32)
        return discrete(closed_form_transform(r) if pos < len(rec) else f32(0))

    def n_step_value(self, g, pos):
        rec, n, disc = self.records[g], self.cfg.n_step, float(self.cfg.discount)
        assert pos < len(rec)
        boot = pos + n + (self.wrong == "nstep_off_by_one")
        has_l = lambda i: "L" in rec.moves[i][2]
        if boot < len(rec) and (not has_l(boot) or self.wrong == "bootstrap_at_l"):
            bootstrap = f32(math.pow(disc, boot - pos) * float(stof(rec.info(boot, "V"))))  # pow(float, int) is double; double * float; stored as float
        else:
            bootstrap = f32(0)
        value = f32(0)
        for i in range(pos, min(boot, len(rec))):
            if has_l(i) and int(rec.info(i, "L")) > 0 and self.wrong != "l_cut_ignored":
                return value
            value = f32(float(value) + math.pow(disc, i - pos) * float(stof(rec.info(i, "R"))))
        return f32(value + bootstrap)

    def action_plane(self, g, pos, rot):
        """the action features of the move at `pos`, or None past the end of the game (see check_absorbing_plane)"""
        rec, cfg = self.records[g], self.cfg
        assert cfg.game != "havannah", "HavannahEnvLoader::getActionFeatures() is not implemented"
        if pos >= len(rec):
            return None
        out, a = np.zeros(cfg.action_size, np.float32), rec.actions[pos]
        if cfg.game == "atari":
            out[a * HIDDEN:(a + 1) * HIDDEN] = 1
        elif not (cfg.game in WITH_PASS and a == cfg.points):
            out[a if self.wrong == "action_not_rotated" else self.rotate_action(a, rot)] = 1
        return out

    def check_absorbing_plane(self, plane, g):
        """what the action features past the end of game g satisfy whatever the reference's generator draws; returns a complaint or None"""
        cfg, plane = self.cfg, np.asarray(plane)
        if not set(np.unique(plane)) <= {0.0, 1.0}:
            return "values other than 0 and 1"
        ones = np.nonzero(plane)[0]
        if cfg.game == "atari":
            a = ones[0] // HIDDEN if len(ones) else -1
            return None if len(ones) == HIDDEN and (ones == np.arange(a * HIDDEN, (a + 1) * HIDDEN)).all() else "not one whole plane of ones"
        if cfg.game in WITH_PASS:
            limit = min(len(self.records[g]), cfg.points)
            return None if len(ones) == 0 or (len(ones) == 1 and ones[0] < limit) else f"more than one 1, or one at an index not below {limit}"
        return None if len(ones) == 1 else f"{len(ones)} ones where a game without a pass has exactly one"

    # ---- planes --------------------------------------------------------------------------------------------------------------------------------------
    def planes(self, g, pos, rot=0):
        cfg, rec = self.cfg, self.records[g]
        pos = min(pos, len(rec))
        if cfg.game == "atari":
            return self.atari_planes(g, pos)
        assert cfg.game in RULES, f"no Python rules model of {cfg.game}"
        if g not in self._planes:
            env = rule_envs.RuleEnv(cfg.conf)
            per_pos = [env.features()]
            for i, (letter, a, _) in enumerate(rec.moves):
                assert letter == "BW"[env.turn() - 1], f"game {g}: move {i} out of turn"
                env.act(a, env.turn())
                per_pos.append(env.features())
            self._planes[g] = per_pos
        f0 = self._planes[g][pos]
        if rot == 0 or cfg.game not in ROTATING:
            return f0
        return f0.reshape(-1, cfg.points)[:, _source(REVERSED[rot], cfg.n)].reshape(-1)

    def screens(self, g):
        """observations_ of atari.cpp:237-249: one entry per position 0 .. moves, None where the record keeps no screen"""
        if g not in self._screens:
            rec = self.records[g]
            obs, raw = [None] * (len(rec) + 1), rec.tags.get("OBS", "")
            if raw:
                frames = np.frombuffer(gzip.decompress(bytes.fromhex(raw)), np.uint8).reshape(-1, 3 * RES * RES)
                assert len(frames) <= len(obs)
                first = 0 if self.wrong == "screens_from_start" else len(obs) - len(frames)
                obs[first:first + len(frames)] = list(frames)
            self._screens[g] = obs
        return self._screens[g]

    def atari_planes(self, g, pos, replay=False):
        rec, obs = self.records[g], self.screens(g)
        if replay or any(obs[i] is None for i in range(max(0, pos - HIST + 1), pos + 1)):
            env = AtariSynth(int(rec.tags["SD"]), self.cfg.episode_length)  # getFeaturesByReplay
            for a in rec.actions[:pos]:
                env.act(a)
            return env.features()
        out = np.zeros((HIST, 4, RES * RES), np.float32)
        for k, i in enumerate(range(pos - HIST + 1, pos + 1)):
            a = 0 if i - 1 < 0 else rec.actions[i - 1]
            out[k, 0] = f32(a) / f32(ATARI_ACTIONS)
            if i >= 0:
                out[k, 1:] = (obs[i].astype(np.float32) / f32(255)).reshape(3, RES * RES)
        return out.reshape(-1)

    def feature_rotations(self, g, pos, planes):
        """Rf: the rotations under which the model's planes are `planes`"""
        return [r for r in self.cfg.rotations if np.array_equal(self.planes(g, pos, r), planes)]

    # ---- priorities ----------------------------------------------------------------------------------------------------------------------------------
    def raw_priority(self, g, pos):
        if self.cfg.game != "atari":
            return f32(1)
        rec = self.records[g]
        return f32(math.fabs(float(f32(self.n_step_value(g, pos) - stof(rec.info(pos, "V"))))) + 1e-6)

    def position_priority(self, g, pos):
        return f64(math.pow(float(self.raw_priority(g, pos)) if self.cfg.per else 1.0, float(self.cfg.alpha)))

    def probability(self, g, pos):
        total = sum(self.game_prio, f64(0))
        return self.prio[g][pos] / total

    def loss_scale(self, g, pos):
        if not self.cfg.per:
            return f64(1)
        if self.sum == 0:
            return f64(0)
        return f64(math.pow(self.num_data() * float(self.prio[g][pos]) / float(self.sum), -float(self.cfg.beta)))

    def scale_bound(self):
        """relative bound between the float64 loss scale and the reference's float one: (N + 16) * 2^-24, N = the positions summed"""
        return (self.num_data() + 16) * 2.0 ** -24

    def update_priority(self, sampled_index, values):
        """values[step][b] on the transformed scale, as the trainer hands them back"""
        values = np.asarray(values, np.float32).reshape(self.cfg.unroll + 1, -1)
        for b, (g, pos) in enumerate(np.asarray(sampled_index).reshape(-1, 2)):
            g, pos = int(g), int(pos)
            rec = self.records[g]
            for step in range(self.cfg.unroll + 1):
                if pos + step < len(rec):
                    v = closed_form_invert(values[step, b])
                    rec.moves[pos + step][2]["V"] = repr(float(v)) if self.wrong == "priority_without_text" else to_string(v)
            self.prio[g][pos] = f64(math.pow(float(self.raw_priority(g, pos)), float(self.cfg.alpha)))
        self.game_prio = [sum(p, f64(0)) for p in self.prio]
        self.sum = sum(self.game_prio, f64(0))

    # ---- one sample against the model ----------------------------------------------------------------------------------------------------------------
    def explain(self, g, pos, rots, action_features, policy, value, reward):
        """Whether ONE rotation of `rots` explains the sample's policy and in-game action planes, and whether value, reward and the planes past the end hold.
        Returns (rotation or None, [complaints])."""
        cfg, U = self.cfg, self.cfg.unroll
        bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
        pol = np.asarray(policy, np.float32).reshape(U + 1, cfg.policy_size)
        act = np.asarray(action_features, np.float32).reshape(-1)[:U * cfg.action_size].reshape(U, cfg.action_size)
        bad = []
        want_v = np.concatenate([self.value(g, pos + s) for s in range(U + 1)])
        if not np.array_equal(bits(want_v), bits(np.asarray(value).reshape(-1)[:want_v.size])):
            bad.append("value")
        if U:
            want_r = np.concatenate([self.reward(g, pos + s) for s in range(U)])
            if not np.array_equal(bits(want_r), bits(np.asarray(reward).reshape(-1)[:want_r.size])):
                bad.append("reward")
        for s in range(U):
            if pos + s >= len(self.records[g]):
                why = self.check_absorbing_plane(act[s], g)
                if why:
                    bad.append(f"action_features past the end, step {s}: {why}")
        found, why_not = None, {}
        for r in rots:
            miss = [f"policy step {s}" for s in range(U + 1) if not np.array_equal(bits(self.policy(g, pos + s, r)), bits(pol[s]))]
            miss += [f"action_features step {s}" for s in range(U) if pos + s < len(self.records[g]) and not np.array_equal(bits(self.action_plane(g, pos + s, r)), bits(act[s]))]
            if not miss:
                found = r
                break
            why_not[r] = miss
        if found is None:
            bad.append(f"no rotation of {list(rots)} explains policy and action_features: {why_not}")
        return found, bad


@lru_cache(None)
def _source(rot, n):
    return np.array([rotate_pos(rot, p, n) for p in range(n * n)])


def discrete(value):
    """toDiscreteValue (atari.cpp:279-293)"""
    value = f32(value)
    out = np.zeros(BINS, np.float32)
    lo, hi = int(math.floor(float(value))), int(math.ceil(float(value)))
    shift = BINS // 2
    lo_s, hi_s = min(max(lo + shift, 0), BINS - 1), min(max(hi + shift, 0), BINS - 1)
    if lo == hi:
        out[lo_s] = 1
    else:
        out[lo_s] = f32(f32(hi) - value)
        out[hi_s] = f32(value - f32(lo))
    return out
