#!/usr/bin/env python3
"""Event model of one launch of sim_kernel<9,9,20,64,2> on one XCD: when does the last game end, under the tail-help rules with and without lending?

    tools/launch_model.py profiles/r15_sim_prof_before.txt [--lead 4 8 16] [--games 32] [--sims 384] [--seeds 20]

The phase times come from a MZ_SIM_PROF dump (the text the worker prints when it closes): walk + leaf, the tower alone, with one helper and with three, the
heads, the exposed backup, and the share of terminal leaves.  Every game draws its own probability of a terminal leaf from a Beta distribution with the dump's
mean (terminal leaves skip tower and heads, which is what makes the games of a launch cost differently), and plays `sims` simulations as a chain of phases:

    tree (walk, leaf, backup) -> tower (solo, pair or quad) -> heads

Tail help (sim_help.h): a game that has finished looks for the running game of least progress that has no helper and at least `min_left` simulations left and takes
its slot 1; if there is none, a free slot 2 or 3 of a helped game.  A helper stays until its game is done.  Slot 1 alone makes a pair tower, all three a quad tower;
a claim counts from the next simulation on.

Lending: a game without a helper opens an offer `--open-delay` us into its tree phase (wave 7 arrives there behind its share of the candidate sort) and closes it
at the end of the walk, `--leaf` us before the end of the tree phase.  A game that is in the same window of its own simulation, has no helper, leads by at least
`lead` simulations and has not taken an offer in this simulation takes the open offer of least progress.  The tower starts when both have finished their tree
phases and is a pair tower; the lender then runs its own tower.  An offer of a game whose leaf turns out terminal is withdrawn at the end of its tree phase.

Three parameters are NOT read from the dump, which does not hold them; they are set by hand and can be given on the command line:
  --beta-a 0.8     the spread of the games' terminal-leaf probabilities within one launch (the second Beta parameter follows from the dump's mean share: 3.4 at 18.7 %).
                   The dump has no per-game, per-launch shares; 0.8 is the value with which the tail-help-only run reproduces the dump's launch: last game at 59.4 ms
                   against 60.1 measured for the 384-simulation launch, mean end / last end 0.89 against 0.87
  --leaf 3.7       us of the tree phase behind the walk: the Go leaf's first half, 8.1 us of the whole leaf less the 4.4 us that run beside the heads
  --open-delay 4.0 us from the end of the heads to wave 7's arrival in front of the next barrier: the gather (0.7 us) and its shares of the rank sort (3.8 us on one wave,
                   DESIGN 3.1 round 2, less on four) and the waits between them; not measured on its own — with 2 and with 6 us the predicted gain at lead 16 is 1.85 and 1.74 % (10 seeds), about as far apart as two sets of seeds

Prints the predicted end of the launch per variant (mean over the seeds) and the towers lent per game.  Standard library only; no GPU."""
import argparse
import heapq
import random
import re
import sys


def read_dump(path):
    text = open(path).read()

    def f(pattern, default=None):
        m = re.search(pattern, text)
        if not m:
            if default is None:
                raise SystemExit(f"{path}: no line matches /{pattern}/")
            return default
        return float(m.group(1))
    return {
        "tree": f(r"select\+leaf\s+avg\s+([0-9.]+) us"),
        "backup": f(r"cand\+expand\s+avg\s+([0-9.]+) us"),
        "heads": f(r"per simulation that ran them: tower [0-9.]+ us, heads ([0-9.]+) us"),
        "solo": f(r"us with a helper, ([0-9.]+) us alone"),
        "pair": f(r"with three helpers, ([0-9.]+) us with\s+one"),
        "quad": f(r"tower ([0-9.]+) us with three helpers"),
        "p_term": f(r"simulations \(([0-9.]+) %; the game with the most") / 100.0,
        "measured_last": f(r"mean [0-9.]+ us, last ([0-9.]+) us", 0.0),
        "measured_mean": f(r"mean ([0-9.]+) us, last", 0.0),
        "launches": f(r"launches: ([0-9]+),", 0.0),
    }


class Game:
    __slots__ = ("p", "done", "t_end", "helpers", "pending", "lender", "taken", "tree_end", "term", "open", "lent", "scan")

    def __init__(self, p):
        self.p, self.done, self.t_end = p, 0, None
        self.helpers, self.pending = 0, 0  # helper slots in effect / claimed (in effect from the next simulation)
        self.lender, self.taken = None, None  # who took this simulation's offer / whose offer this game took
        self.tree_end, self.term, self.open, self.scan, self.lent = 0.0, False, False, False, 0


def run(par, games, sims, lead, min_left, open_delay, leaf, beta_a, seed):
    rng = random.Random(seed)
    beta_b = beta_a * (1.0 - par["p_term"]) / max(1e-9, par["p_term"])
    G = [Game(rng.betavariate(beta_a, beta_b)) for _ in range(games)]
    ev, n = [], 0

    def push(t, kind, g):
        nonlocal n
        n += 1
        heapq.heappush(ev, (t, n, kind, g))

    def start_sim(t, g):
        g.helpers = g.pending
        g.term = rng.random() < g.p
        g.tree_end = t + par["tree"] + par["backup"]
        g.lender, g.taken, g.open, g.scan = None, None, False, False
        if lead and g.helpers == 0:
            push(min(t + open_delay, g.tree_end - leaf), "open", g)
            push(g.tree_end - leaf, "close", g)
        push(g.tree_end, "tree", g)

    def match(t, lender, owner):
        owner.lender, lender.taken, owner.open, lender.scan = lender, owner, False, False

    def tower(g):
        return par["quad"] if g.helpers == 3 else par["pair"] if g.helpers >= 1 else par["solo"]

    def find_help(t):  # a finished CU looks for a game to help
        run_ = [g for g in G if g.t_end is None and sims - g.done >= min_left]
        first = [g for g in run_ if g.pending == 0]
        more = [g for g in run_ if 0 < g.pending < 3]
        for cands in (first, more):
            if cands:
                min(cands, key=lambda g: g.done).pending += 1
                return True
        return False

    idle = 0
    for g in G:
        start_sim(0.0, g)
    while ev:
        t, _, kind, g = heapq.heappop(ev)
        if kind == "open":
            if g.pending == 0 and g.lender is None:
                g.open = True
                takers = [l for l in G if l.scan and l.taken is None and l.done - g.done >= lead and sims - g.done >= min_left]
                if takers:
                    match(t, max(takers, key=lambda l: l.done), g)
                # ... and its own look at the others' offers: only a game whose offer nobody has taken
            if g.lender is None and g.helpers == 0:
                g.scan = True
                offers = [o for o in G if o.open and o is not g and g.done - o.done >= lead and sims - o.done >= min_left]
                if offers:
                    g.open = False  # (it closes its own offer before it takes one)
                    match(t, g, min(offers, key=lambda o: o.done))
        elif kind == "close":
            g.open, g.scan = False, False
        elif kind == "tree":
            if g.taken is not None:  # a lender: one tower of the other game first (or the news that it has none), then its own
                o = g.taken
                both = max(g.tree_end, o.tree_end)
                if t < both:
                    push(both, "tree", g)
                    continue
                g.taken = None
                if not o.term:
                    g.lent += 1
                    push(t + par["pair"], "tree", g)
                    continue
            if g.term:
                push(t, "sim", g)
            elif g.lender is not None:
                push(max(t, g.lender.tree_end) + par["pair"] + par["heads"], "sim", g)
            else:
                push(t + tower(g) + par["heads"], "sim", g)
        elif kind == "sim":
            g.done += 1
            if g.done < sims:
                start_sim(t, g)
            else:
                g.t_end = t
                idle += 1 + g.helpers  # its own CU and its helpers' look for another game
                while idle > 0 and find_help(t):
                    idle -= 1
    ends = [g.t_end for g in G]
    return max(ends), sum(ends) / len(ends), sum(g.lent for g in G) / len(G)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dump", help="a MZ_SIM_PROF dump taken WITHOUT lending (MZ_NO_SPEC=256, or a build from before it)")
    ap.add_argument("--lead", type=int, nargs="*", default=[4, 8, 16])
    ap.add_argument("--games", type=int, default=32, help="games of one XCD")
    ap.add_argument("--sims", type=int, default=384)
    ap.add_argument("--min-left", type=int, default=2)
    ap.add_argument("--open-delay", type=float, default=4.0, help="us from the start of a simulation's tree phase to its offer")
    ap.add_argument("--leaf", type=float, default=3.7, help="us of the tree phase behind the walk (the leaf's first half): the offer is closed in front of it")
    ap.add_argument("--beta-a", type=float, default=0.8, help="first parameter of the Beta distribution of a game's terminal-leaf probability (the second follows from the dump's mean)")
    ap.add_argument("--seeds", type=int, default=20)
    a = ap.parse_args()
    par = read_dump(a.dump)
    print("phase times (us): " + ", ".join(f"{k} {par[k]:.2f}" for k in ("tree", "backup", "solo", "pair", "quad", "heads")) + f"; terminal leaves {100 * par['p_term']:.2f} %")
    base = None
    for lead in [0] + a.lead:
        res = [run(par, a.games, a.sims, lead, a.min_left, a.open_delay, a.leaf, a.beta_a, s) for s in range(a.seeds)]
        last, mean, lent = (sum(r[i] for r in res) / len(res) for i in range(3))
        base = base or last
        name = "tail help only" if lead == 0 else f"lending, lead {lead}"
        print(f"{name:22s}: last game ends at {last / 1e3:7.2f} ms, mean {mean / 1e3:7.2f} ms (mean / last {mean / last:.3f}), {lent:5.1f} towers lent per game"
              + ("" if lead == 0 else f" -> {100 * (base - last) / base:+.2f} %"))
    if par["measured_last"]:
        print(f"measured ({int(par['launches'])} launches of the dump, all sizes): mean {par['measured_mean'] / 1e3:.2f} ms, last {par['measured_last'] / 1e3:.2f} ms "
              f"(mean / last {par['measured_mean'] / par['measured_last']:.3f})")
    return 0


if __name__ == "__main__":
    sys.exit(main())
