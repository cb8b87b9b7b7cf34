"""A plain model of match play (mz_worker_create_match) over the search model of tests/search_model.py: the schedule — two lanes, the step
counter, the colour rule, serial numbers, filler games, the end of the match —, per move S.search with the network of the side to move, and the tally.  The
environment and the two networks are handed in; this file imports neither the oracle nor the product.

The schedule, in the words of the issue: the G slots are two lanes of G / 2 (slot s lies in lane s // (G / 2)); t counts the steps, one move of every game
each.  A game that starts in lane h at step t0 has side (h + t0) mod 2 as its first player (side 0 is A, side 1 is B), so in step t its side to move is
(first + t - t0) mod 2 = (h + t) mod 2: all games of a lane share it.  A game gets its serial number when it starts, in slot order within a step, while
fewer than N have started; a slot that frees up later plays an uncounted filler.  The match is over after the step in which the N-th counted game finished.

Three deliberately WRONG readings are selectable, so that a test can show that its inputs tell them from the right one (tests/test_match_model.py):
swapped = the two networks exchanged, colour_blind = a restarted game always has A as its first player, nets handed in as (A, A) = one network for both."""
import search_model as S

SIDES = ("A", "B")


class Slot:
    def __init__(self, slot, lane):
        self.slot, self.lane = slot, lane
        self.serial, self.t0, self.first = -1, 0, 0
        self.env, self.moves = None, []


class Schedule:
    """the bookkeeping alone: who moves, who starts, which games count, when the match ends"""

    def __init__(self, G, N, colour_blind=False):
        assert G >= 2 and G % 2 == 0 and N >= G
        self.G, self.N, self.t, self.colour_blind = G, N, 0, colour_blind
        self.slots = [Slot(s, s // (G // 2)) for s in range(G)]
        self.stats = dict(games_started=0, games_finished=0, moves=0, filler_games=0, a_first=[0, 0, 0], a_second=[0, 0, 0], resignations=0, steps=0, done=False)
        self.finished = []  # (serial, slot, first side, t0, step it ended in), in the order the lines leave
        self.fillers = []   # (slot, t0)
        for sl in self.slots:
            self._start(sl, 0, restart=False)

    def _start(self, sl, t0, restart=True):
        sl.t0, sl.moves = t0, []
        sl.first = 0 if (restart and self.colour_blind) else (sl.lane + t0) % 2
        if self.stats["games_started"] < self.N:
            sl.serial = self.stats["games_started"]
            self.stats["games_started"] += 1
        else:
            sl.serial = -1
            self.stats["filler_games"] += 1
            self.fillers.append((sl.slot, t0))

    def side_to_move(self, sl):
        return (sl.first + self.t - sl.t0) % 2

    def colour_to_move(self, sl):
        return S.BLACK if (self.t - sl.t0) % 2 == 0 else S.WHITE

    def end_step(self, results):
        """results[slot] = (moved, ended, score of the first player's colour as outputGame prints it, resigned); slots in order.  Returns the slots that
        restarted, and sets stats['done'] after the step in which the N-th counted game finished"""
        restarted = []
        for sl in self.slots:
            moved, ended, score, resigned = results[sl.slot]
            if sl.serial >= 0 and moved:
                self.stats["moves"] += 1
            if not ended:
                continue
            if sl.serial >= 0:
                first = 0 if score > 0 else (2 if score < 0 else 1)
                if sl.first == 0:
                    self.stats["a_first"][first] += 1
                else:
                    self.stats["a_second"][2 - first] += 1
                self.stats["games_finished"] += 1
                self.stats["resignations"] += int(resigned)
                self.finished.append((sl.serial, sl.slot, sl.first, sl.t0, self.t))
            self._start(sl, self.t + 1)
            restarted.append(sl)
        self.t += 1
        self.stats["steps"] = self.t
        self.stats["done"] = self.stats["games_finished"] >= self.N
        return restarted


def run_schedule(G, N, games, colour_blind=False):
    """The schedule on scripted games: `games` lists (length, score) of the games in the order they start (the first G are the slots' first games, then the
    restarts in step and slot order); every game ends on the board, none resigns.  Returns the Schedule after the match."""
    sch = Schedule(G, N, colour_blind)
    it = iter(games)
    for sl in sch.slots:
        sl.script = next(it)
    while not sch.stats["done"]:
        results = {}
        for sl in sch.slots:
            length, score = sl.script
            results[sl.slot] = (True, sch.t - sl.t0 + 1 == length, score, False)
        for sl in sch.end_step(results):
            sl.script = next(it)
    return sch


def p_string(cfg, t, gz):
    """the P tag of a PUCT root as the worker prints it (child order); a Gumbel root's is an unordered_map's iteration: its dictionary instead"""
    if cfg.actor_use_gumbel:
        return gz.policy(t)
    return ",".join(f"{t.action[c]}:{'%g' % float(t.count[c])}" for c in t.kids(0) if t.count[c] != 0)


def game_line(sl, names, score, terminal):
    """what a test reads off a `Match` line: its head, the tags the match decides, and the moves"""
    n = len(sl.moves)
    re_tag = ("%f" % float(score)) if terminal else ("%g" % float(score))  # std::to_string of the result on the board; an ostream of the resigner's loss
    return dict(head=f"Match true {n} {n} {'%g' % float(score)}", RE=re_tag, DLEN=f"0-{n - 1}", PB=names[sl.first], PW=names[1 - sl.first],
                moves=list(sl.moves), serial=sl.serial, slot=sl.slot)


def play_match(cfg, make_env, nets, G, N, names=SIDES, muzero=False, resign_enabled=True, swapped=False, colour_blind=False, max_steps=None, choose=None):
    """The whole match.  make_env() gives a game at its start; nets = (side A's, side B's) behind the network interface of S.search.  choose(slot, tree)
    replaces the decision (a test that replays the worker's random selection); None: S.search's own (by count).  Returns (lines, stats, slots): the counted
    games in the order their lines leave (game_line), the tally, and the slots as the match left them (or as max_steps steps left them)."""
    if swapped:
        nets = (nets[1], nets[0])
    sch = Schedule(G, N, colour_blind)
    for sl in sch.slots:
        sl.env = make_env()
    lines = []
    while not sch.stats["done"] and (max_steps is None or sch.t < max_steps):
        results = {}
        for sl in sch.slots:
            # (the worker checks the same every step and stops with MZ_ERR_STATE; under colour_blind the lane's games stop sharing their side, not their colour)
            assert sl.env.turn() == sch.colour_to_move(sl), (sl.slot, sch.t, sl.t0)
            colour = sl.env.turn()
            t, sel, gz = S.search(cfg, sl.env, nets[sch.side_to_move(sl)], muzero)
            if choose is not None:
                sel = choose(sl, t)
            resign = resign_enabled and t.is_resign(sel)
            moved = False
            if not resign:
                sl.env.act(t.action[sel], t.player[sel])
                sl.moves.append(("B" if colour == S.BLACK else "W", t.action[sel], p_string(cfg, t, gz), t.root_value_string(), "%g" % float(sl.env.reward())))
                moved = True
            ended = resign or sl.env.terminal()
            score = 0.0
            if ended:
                # evalScore(!isTerminal()): the result on the board, or the loss of the player to move who resigned (base_env.h: Black resigns -> -1)
                score = float(sl.env.eval_score()) if not resign else (-1.0 if sl.env.turn() == S.BLACK else 1.0)
                if sl.serial >= 0:
                    lines.append(game_line(sl, names, score, not resign))
            results[sl.slot] = (moved, ended, score, resign)
        for sl in sch.end_step(results):
            sl.env = make_env()
    return lines, dict(sch.stats), sch.slots
