"""The lattice of the log-mel edge tests (test_logmel_edges.py on the simulator, test_gpu_logmel_edges.py on the device): twelve
shapes chosen by the path they send k_logmel down, a restatement of the kernel's dispatch from the rule's numbers that says
which path that is, the coverage the lattice must keep, a window that weighs the last k terms fully, and the stream lengths and
chain splits both files use."""
import numpy as np

from logmel_util import CONFIGS, F, chain_splits, sim_rule
from test_gpu_logmel import edge_lengths

TILE, WAVES, NT, DEPTH = 32, 4, 4, 4          # LM_TILE, LM_WAVES, LM_NT of logmel.h; the k steps lm_tiles pipelines at a time


def _shape(n_fft, hop, n_mels, sample_rate, slaney=False):
    return dict(sample_rate=sample_rate, n_fft=n_fft, hop=hop, n_mels=n_mels, f_min=0.0, f_max=0.0, mel_scale="slaney" if slaney else "htk",
                mel_norm="slaney" if slaney else "none")


# number -> config; what each row is there for stands next to it and is asserted by coverage() below
LATTICE = {
    1: _shape(34, 17, 5, 8000),                   # tail 1; odd hop = n_fft / 2
    2: _shape(36, 1, 7, 8000),                    # tail 2; hop 1; 7 * 32 items < 256 threads
    3: _shape(38, 6, 8, 8000),                    # tail 3; hop = 2 mod 4
    4: _shape(62, 12, 16, 8000),                  # a full last tile; sh 2; tail 3
    5: _shape(128, 64, 40, 16000),                # 5 tiles: wave 0 nv 2, the others nv 1; sh 6
    6: _shape(254, 100, 64, 16000, True),         # 8 tiles, full: every wave nv 2; tail 3
    7: _shape(256, 80, 32, 16000),                # 9 tiles: nv 3 and 2; the Nyquist pair alone in its tile; sh 4
    8: _shape(638, 319, 80, 22050, True),         # 20 tiles: second round nv 1 in every wave; odd hop
    9: _shape(766, 250, 128, 44100),              # 24 tiles: second round nv 2
    10: _shape(894, 444, 256, 48000),             # 28 tiles: second round nv 3; n_mels 256; empty bands
    11: _shape(1024, 512, 80, 48000, True),       # the largest LDS tile; sh 9; three rounds
    12: _shape(1022, 510, 1, 48000),              # 32 tiles = two full rounds; n_mels 1; the largest unskewed tile
}
NUMBERS = list(LATTICE)
IDS = ["%d_%d_%d_%d" % (k, c["n_fft"], c["hop"], c["n_mels"]) for k, c in LATTICE.items()]
# live bands where a filter is narrower than a bin; every band elsewhere.  Shape 6's 64 Slaney bands are all live; its HTK
# variant ("6h": the value and table tests run it as well) has one empty band under 8 full tiles.
LIVE_BANDS = {5: 39, "6h": 63, 9: 125, 10: 228}
VARIANTS = {"6h": _shape(254, 100, 64, 16000)}
VALUE_SHAPES = NUMBERS + list(VARIANTS)
VALUE_IDS = IDS + ["6h_254_100_64_htk"]
CHAIN_SHAPES = [1, 2, 3, 4, 6]
SINGLE_SAMPLE_ON_DEVICE = [1, 3]


def shape(number):
    return LATTICE[number] if number in LATTICE else VARIANTS[number]


def dispatch(rule):
    """what lm_wg_dft / lm_tiles do with a rule, from sim_rule's numbers only: dict(tail, groups, hop_class, full)
    tail: k steps left to the loop behind the pipeline, half % DEPTH
    groups: the set of (round, nv) over the four waves: wave w takes the tiles g, g + WAVES, .. of g = w + round WAVES NT, nv of
            them at once, nv = min(NT, ceil((tiles - g) / WAVES))
    hop_class: "odd", "2mod4" (both unskewed) or the skew's shift sh
    full: the Nyquist pair fills the last tile's last two columns, no zero column behind it"""
    half, tiles = rule["bins"] - 1, rule["cols"] // TILE
    groups = set()
    for wave in range(WAVES):
        for rnd, g in enumerate(range(wave, tiles, WAVES * NT)):
            groups.add((rnd, min(NT, (tiles - g + WAVES - 1) // WAVES)))
    if rule["sh"] == 31:
        hop_class = "odd" if rule["fstride"] & 1 else "2mod4"       # unskewed: fstride is the hop
    else:
        hop_class = rule["sh"]
    return dict(tail=half % DEPTH, groups=groups, hop_class=hop_class, full=2 * rule["bins"] == rule["cols"])


REQUIRED = [("tail", t) for t in range(DEPTH)] + [("group", (r, nv)) for r in (0, 1) for nv in range(1, NT + 1)] + [("rounds", 3)] + \
    [("hop_class", c) for c in ["odd", "2mod4"] + list(range(2, 10))] + [("full", True), ("full", False)]


def coverage(configs):
    """the set of REQUIRED's items the configs reach"""
    seen = set()
    for cfg in configs:
        d = dispatch(sim_rule(**cfg))
        seen.add(("tail", d["tail"]))
        seen.update(("group", g) for g in d["groups"])
        seen.add(("rounds", 1 + max(r for r, _ in d["groups"])))
        seen.add(("hop_class", d["hop_class"]))
        seen.add(("full", d["full"]))
    return seen


def all_configs():
    return list(CONFIGS.values()) + list(LATTICE.values())


def rising(n_fft):
    """a rising window that is not symmetric: the last k terms, the ones lm_tiles' tail loop adds, carry full weight (under the
    periodic Hann window they are weighted almost to nothing)"""
    return np.linspace(0.05, 1.0, n_fft).astype(np.float32)


WINDOWS = ["hann", "rising"]


def window_of(name, n_fft):
    return None if name == "hann" else rising(n_fft)


def stream_lengths(n_fft, hop):
    """n_fft <= 256: 0, h, h + 1, 3 hop + h -+ 1 samples and END frame counts F - 1, F, F + 1, 2 F + 1; above that 0, h, h + 1 and
    the F and F + 1 streams only, so that the simulator's scalar chain stays short"""
    lengths = edge_lengths(n_fft, hop)
    return lengths if n_fft <= 256 else lengths[:3] + lengths[6:8]


def lattice_row(n_fft):
    """not a multiple of 32: one block holds both frames and padding"""
    return 2 * F + 3 if n_fft <= 256 else F + 3


DTYPE_NAMES, LAYOUT_NAMES, SCALE_NAMES = ["float32", "float16", "bfloat16"], ["mel_major", "time_major"], ["log10", "power", "db", "log"]


def lattice_output(number, end, window):
    """(dtype, layout, scale) of a lattice run: the types and layouts mixed over the lattice, float32 in at least one run of every
    shape; shapes 1 and 2 (n_mels 5 and 7, coprime to 32) always time_major"""
    e, w = int(bool(end)), WINDOWS.index(window)
    layout = "time_major" if number <= 2 else LAYOUT_NAMES[(number + e) % 2]
    return DTYPE_NAMES[(number + e + w) % 3], layout, SCALE_NAMES[(number + 2 * w + e) % 4]


def carry_split(n_fft, hop):
    """[N, n - N] of chain_splits' stream with N >= n_fft the smallest with (N - h) % hop == hop - 1: the next frame starts at
    N - n_fft + 1, so the carry behind the first call holds exactly n_fft - 1 samples, its cap"""
    n, h = 7 * hop + n_fft, n_fft // 2
    N = next(N for N in range(n_fft, n) if (N - h) % hop == hop - 1)
    return [N, n - N]


def edge_splits(n_fft, hop, singles=True):
    """(n, splits): chain_splits' list, the n_fft - 1 carry and (singles) the split into single samples"""
    n, splits = chain_splits(n_fft, hop)
    splits = splits + [carry_split(n_fft, hop)]
    if singles:
        splits.append([1] * n)
    return n, splits


def chain_row(n_fft, hop):
    return (7 * hop + n_fft) // hop + 2
