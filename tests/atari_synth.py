"""The synthetic Atari-shaped game (oracle/o_env.cpp AtariSynthEnv, the product's twin in env.cpp) in plain Python, behind the environment interface of
tests/search_model.py.  It keeps the feature contract of the reference's Atari environment (environment/atari/atari.h:17-27,40,75 and atari.cpp:48-131): one
player, 18 actions that are always legal, features of the last 8 steps as [one plane action id / 18, R, G, B / 255] oldest first and zeros before the start,
action features 18 x 6 x 6 with plane `action id` all ones, the cumulative reward as the score.  Screens and rewards are counter hashes of (seed, step); the
seed of a game is the SD tag of its record.  tests/test_search_model.py pins this file to the oracle's environment bit for bit."""
import numpy as np

f32 = np.float32
M64 = (1 << 64) - 1
RES, HIST, ACTIONS, BLOCK = 96, 8, 18, 8


def amix(z):
    """the finaliser of splitmix64 on a 64-bit word"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class AtariSynth:
    def __init__(self, seed, episode_length):
        self.seed, self.episode_length = int(seed), int(episode_length)
        self.useed = self.seed & 0xFFFFFFFF  # static_cast<uint32_t>(seed_)
        self.actions, self.last_reward, self.total = [], f32(0), f32(0)
        self.screens = [np.zeros((3, RES, RES), np.float32)] * (HIST - 1) + [self.screen(0)]
        self.action_planes = [f32(0)] * HIST

    def clone(self):
        c = AtariSynth.__new__(AtariSynth)
        c.__dict__.update(self.__dict__)
        c.actions, c.screens, c.action_planes = list(self.actions), list(self.screens), list(self.action_planes)
        return c

    def num_players(self): return 1
    def turn(self): return 1
    def legal(self): return [1] * ACTIONS
    def terminal(self): return len(self.actions) >= self.episode_length
    def reward(self): return self.last_reward
    def eval_score(self): return self.total

    def screen(self, step):
        """one hashed byte per 8 x 8 block per colour plane, as float32 byte / 255"""
        nb = RES // BLOCK
        base = self.useed * 0xD1B54A32D192ED03 + step * 0x100000001B3
        b = np.array([amix(base + k * 0x9E3779B97F4A7C15) >> 56 for k in range(3 * nb * nb)], np.float32).reshape(3, nb, nb)
        return np.repeat(np.repeat(b, BLOCK, axis=1), BLOCK, axis=2) / f32(255)

    def act(self, a, player=1):
        assert 0 <= a < ACTIONS and player == 1
        step = len(self.actions) + 1
        hit = (amix(self.useed * 0x9E3779B97F4A7C15 + 0x5157 * step) >> 40) < int(0.05 * (1 << 24))
        self.last_reward = f32(1 if hit else 0)
        self.total = f32(self.total + self.last_reward)
        self.actions.append(a)
        self.action_planes = self.action_planes[1:] + [f32(f32(a) / f32(ACTIONS))]
        self.screens = self.screens[1:] + [self.screen(step)]

    def features(self):
        out = np.empty((HIST, 4, RES, RES), np.float32)
        for i in range(HIST):
            out[i, 0] = self.action_planes[i]
            out[i, 1:] = self.screens[i]
        return out.reshape(-1)

    def action_features(self, a, player=1):
        f = np.zeros((ACTIONS, 36), np.float32)
        f[a] = 1
        return f.reshape(-1)
