"""numpy restatement of csrc/live_compact.hip, shared by tests/test_emu_live_compact.py (CPU interpreter) and
tests/test_gpu_live_samples.py: which samples are live, the offset table, the gathered masks, and the liveness patterns
both files run."""
import numpy as np

from scnerf_amd import mlp_layout as ML


def live_index(d_raw):
    """ascending indices of the rows of d_raw [P, 4] with a non-zero word, the sign bit ignored"""
    w = np.ascontiguousarray(d_raw, np.float32).reshape(-1, 4).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.flatnonzero((w != 0).any(axis=1)).astype(np.int32)


def padded_index(idx, P):
    """live_idx as the kernel leaves it up to the padded count (what lies behind is not written)"""
    out = np.zeros(ML.padded_samples(len(idx)), np.int32)
    out[:len(idx)] = idx
    return out


def xoff_table(idx):
    """entry 16 (k >> 4) + 2 (k & 7) + ((k >> 3) & 1) = byte offset of sample idx[k] in a 256-wide tile-native section"""
    n = ML.padded_samples(len(idx))
    i = padded_index(idx, None).astype(np.int64)
    k = np.arange(n)
    out = np.zeros(n, np.uint32)
    out[(k & ~15) + 2 * (k & 7) + ((k >> 3) & 1)] = ((i >> 5) * 32768 + (i & 31) * 16).astype(np.uint32)
    return out


def gather_masks(masks, P, idx):
    """masks: the nine lane-native sections behind a workspace of P samples, [9][Ppad / 32][lane = 32 h + m][4] words"""
    Pp, Pl = ML.padded_samples(P), ML.padded_samples(len(idx))
    rows = masks.reshape(9, Pp // 32, 2, 32, 4).transpose(0, 1, 3, 2, 4).reshape(9, Pp, 8)[:, idx]
    out = np.zeros((9, Pl, 8), masks.dtype)
    out[:, :len(idx)] = rows
    return out.reshape(9, Pl // 32, 32, 2, 4).transpose(0, 1, 3, 2, 4).reshape(-1)


def patterns(P, seed=0):
    """name -> bool [P]: all live, none, exactly one, alternating, a dead first half, dead runs across the 32-sample tiles,
    the 128-sample blocks and the 1024-sample workgroups of the compaction, and a random 70 %"""
    k = np.arange(P)
    out = {"all": np.ones(P, bool), "none": np.zeros(P, bool), "one": k == (P * 2) // 3, "alternating": k % 2 == 1,
           "dead first half": k >= P // 2}
    runs = np.ones(P, bool)
    for edge in (32, 128, 256, 1024, 2048, 4096):
        runs[max(0, edge - 5):edge + 7] = False
    runs[-3:] = False
    out["dead runs across boundaries"] = runs
    out["random"] = np.random.default_rng(seed).random(P) < 0.7
    return out


def d_raw_with(live, seed=1):
    """d_raw [P, 4] whose rows are live exactly where `live` says: dead rows are +-0, some live rows have a single
    non-zero word (a denormal among them)"""
    rng = np.random.default_rng(seed)
    P = live.shape[0]
    d = rng.standard_normal((P, 4)).astype(np.float32) * 1e-3
    single = rng.random(P) < 0.2
    col = rng.integers(0, 4, P)
    only = np.zeros((P, 4), np.float32)
    only[np.arange(P), col] = np.where(rng.random(P) < 0.5, np.float32(1e-42), np.float32(-2.5))
    d[single] = only[single]
    dead = np.where(rng.random((P, 4)) < 0.5, np.float32(0.0), np.float32(-0.0))
    d[~live] = dead[~live]
    return d
