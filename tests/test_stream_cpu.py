"""The counter-based stream of include/rg_stream.h has one numpy statement (tests/stream_model.py) and one device statement
(robot_gym_amd/csrc/rg_stream_dev.inc).  Known answers that do not come from the code under test, the scalar and the array
forms against each other, and the checks that keep the statement single: every model imports it, the purpose blocks of its
three registered users are disjoint, and its multiplier appears in one file per side."""
import glob
import math
import os

import numpy as np

from robot_gym_amd.core import dr_abi, est_abi, sensor_abi
from tests import ddpg_model, dr_model, episode_model, est_model, policy_model, sensor_model, terrain_model
from tests import stream_model as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1
NEG3 = 2 ** 64 - 3     # the key -3.0 as the device reads it

# (seed, key, draw, purpose, index) -> h, recorded from the models of the commit before there was one statement: sensor_model.hash4,
# dr_model.hash4, policy_model.noise_hash and sensor_model.vhash all gave h, and episode_model.uniform, sensor_model.uniform and
# dr_model.uniform all gave (h >> 11) * 2^-53.  0xff is ix(2^52, 63, 3): k << 12 has wrapped to 0.
CHAINS = [((0, 0, 0, 0, 0), 0x2130748AAAC80268),
          ((1, 2, 3, 4, 5), 0x415CA65FB7064546),
          ((M64, M64, M64, M64, M64), 0x6A4F23D31DB0626A),
          ((0x0123456789ABCDEF, NEG3, 7, 18, 0xFF), 0x17A94FE69AC280CE),
          ((12345, 0, M64, 5, 0), 0xB0F822FDDA1C1C93),
          ((2 ** 63, 2 ** 63, 1, 35, 2 ** 63), 0x353FBA9F8A67DB11),
          ((12345, 5, 0, 2, 0), 0x40153532777E0227)]
UNIFORMS = ["0x1.0983a45556400p-3", "0x1.0572997edc190p-2", "0x1.a93c8f4c76c18p-2", "0x1.7a94fe69ac280p-4", "0x1.61f045fbb4383p-1",
            "0x1.a9fdd4fc533ecp-3"]
# (seed, key, I, J) -> h of the terrain's three words, from terrain_model.hash_words of that commit; words of either sign
TERRAIN = [((0, 0, 0, 0), 0x238275BC38FCBE91), ((7, -1, -2, 3), 0x6B736406D7B8EBD1), ((M64, -(2 ** 63), 2 ** 63 - 1, -1), 0x2D6F562AF40F45CD),
           ((99, 5, -(2 ** 39), 2 ** 39), 0xCFBA2B581BF8A9A5)]
# n of (seed 42, key -3, draw 3, purpose 19) at (k, row), from sensor_model.noise and sensor_model.vnoise of that commit
NOISES = [((0, 0), "0x1.b86bd6a4f5aaep-2"), ((1, 5), "0x1.26535a8f588f4p-4"), ((2 ** 52, 63), "0x1.17a436aca3be7p+0"),
          ((123456789, 1023), "-0x1.976a3dfe65b26p-1")]


def test_known_answers_of_mix_and_the_chain():
    # the first output of splitmix64 seeded with 0 (Vigna's reference implementation): one round of the chain on zero words
    assert S.mix64(S.GOLDEN) == 0xE220A8397B1DCDAF
    assert S.mix64(0) == 0 and S.mix64(M64) == 0xB4D055FCF2CBBD7B
    # by hand for the all-zero words, the one restatement outside the model: four rounds, each h = mix((h ^ 0) + GOLDEN)
    h = 0
    for _ in range(4):
        z = (h + 0x9E3779B97F4A7C15) & M64
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & M64
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & M64
        h = z ^ (z >> 31)
    assert h == S.chain(0, 0, 0, 0, 0) == 0x2130748AAAC80268
    for words, want in CHAINS:
        assert S.chain(*words) == want, words
        assert int(S.vchain(words[0], *(np.array([w], dtype=np.uint64) for w in words[1:]))[0]) == want, words
    for (words, h), u in zip(CHAINS, UNIFORMS):
        assert S.uniform(*words) == float.fromhex(u) == (h >> 11) / 2 ** 53, words
    for words, want in TERRAIN:
        assert S.chain(*words) == want, words
    assert S.chain(5) == 5 and S.chain(-1) == M64     # no word: the seed as a 64-bit word


def test_known_answers_of_the_index_word_the_readings_and_the_noise():
    assert S.ix(3, 19, 2) == 3 * 4096 + 19 * 4 + 2 and S.ix(2 ** 52, 63, 3) == 0xFF and S.ix(2 ** 52 - 1, 0) == 2 ** 64 - 4096
    assert S.words([-3.0, -1.0, 2.0 ** 40, 0.9]).tolist() == [NEG3, M64, 2 ** 40, 0]
    assert S.bounded([np.nan, -3.0, 2.5, 99.0, np.inf], 15).tolist() == [0, 0, 2, 15, 15]
    assert int(S.bounded(2.0 ** 60, 2.0 ** 52)) == 2 ** 52
    for (k, row), want in NOISES:
        n = S.noise(42, NEG3, 3, 19, k, row)
        assert n == float.fromhex(want) and abs(n) < 2.0 * math.sqrt(3.0), (k, row)
        assert float(S.vnoise(42, np.uint64(NEG3), np.uint64(3), 19, np.uint64(k), np.uint64(row))) == n
    # the bound is the sum's: four uniforms in [0, 1) lie within 2 of their mean
    assert S.ROOT3 == math.sqrt(3.0)
    assert [S.delay_draw(9, k, 2, 16, 1, 7) for k in range(8)] == [3, 1, 4, 5, 5, 6, 5, 3]


def test_scalar_and_array_forms_agree():
    rng = np.random.default_rng(0)
    w = np.concatenate([rng.integers(0, 2 ** 64, (300, 5), dtype=np.uint64),
                        np.array([[0] * 5, [M64] * 5, [0, M64, 0, M64, 0], [M64, 0, 2 ** 63, 1, 2 ** 63 - 1]], dtype=np.uint64)])
    assert S.vmix(w[:, 0]).tolist() == [S.mix64(int(z)) for z in w[:, 0]]
    rows = [[int(x) for x in r] for r in w]
    for seed in (0, 12345, M64):
        assert S.vchain(seed, *w[:, 1:].T).tolist() == [S.chain(seed, *r[1:]) for r in rows]
        assert S.vchain(seed, *w[:, 1:4].T).tolist() == [S.chain(seed, *r[1:4]) for r in rows]
        assert S.vuniform(seed, *w[:, 1:].T).tolist() == [S.uniform(seed, *r[1:]) for r in rows]
    k, row = w[:, 3] >> np.uint64(11), w[:, 4] & np.uint64(1023)      # k to 2^53: past the tick bound, where k << 12 wraps
    assert S.vnoise(9, w[:, 1], w[:, 2], 17, k, row).tolist() == [S.noise(9, r[1], r[2], 17, int(a), int(b)) for r, a, b in zip(rows, k, row)]
    u = S.vuniform(3, *w[:, 1:].T)
    assert 0.0 <= u.min() and u.max() < 1.0


def test_every_model_uses_the_one_definition():
    for model in (dr_model, sensor_model, episode_model):
        assert model.mix64 is S.mix64 and model.uniform is S.uniform and model.M64 == S.M64 and model.GOLDEN == S.GOLDEN, model.__name__
    assert dr_model.hash4 is S.chain and sensor_model.hash4 is S.chain and sensor_model.vhash is S.vchain
    for name in ("vmix", "vuniform", "vnoise", "ix", "noise", "delay_draw", "words", "bounded"):
        assert getattr(sensor_model, name) is getattr(S, name), name
    assert est_model.SM is sensor_model
    assert terrain_model.hash_words is S.chain and terrain_model.unit is S.uniform
    assert policy_model.noise_hash is S.chain and ddpg_model.sample_hash is S.chain


def test_the_purpose_blocks_are_pairwise_disjoint():
    blocks = {abi.__name__: {v for n, v in vars(abi).items() if n.startswith("PURPOSE_")} for abi in (dr_abi, sensor_abi, est_abi)}
    assert [len(b) for b in blocks.values()] == [6, 6, 4]
    everything = set().union(*blocks.values())
    assert len(everything) == 16, blocks     # no purpose twice, within a user or between two
    # a user owns the block of 16 it starts in (rg_stream.h, the registry)
    assert [{p // 16 for p in b} for b in blocks.values()] == [{0}, {1}, {2}]


def test_the_stream_constant_appears_once():
    def holders(*patterns):
        paths = [p for pattern in patterns for p in glob.glob(os.path.join(ROOT, pattern))]
        return sorted(os.path.basename(p) for p in paths if "BF58476D1CE4E5B9" in open(p).read().upper())
    assert holders("robot_gym_amd/csrc/*.hip", "robot_gym_amd/csrc/*.inc", "robot_gym_amd/csrc/*.h") == ["rg_stream_dev.inc"]
    # this file names the constant to look for it (and in the one by-hand restatement above); the model is the only other
    assert holders("tests/*.py") == ["stream_model.py", "test_stream_cpu.py"]
