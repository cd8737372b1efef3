"""The size lists (shard bytes per block; a tile is 4096 shard bytes) the
ragged tests share, and the layout arithmetic of a ragged batch."""
import numpy as np

A = [64] * 65                                     # 64 blocks in tile 0, one alone in tile 1
B = [4096, 4096, 4096]                            # every tile exactly one block
C = [4032, 64, 4160, 8256, 64, 0, 192, 0]         # straddles, a three-tile block, zero sizes, partial tail
D = [64]
D1 = [4160]                                       # D'
E = [64 * int(r) for r in np.random.default_rng(7).integers(0, 131, size=200)]
F1 = [192] * 100                                  # uniform
F2 = [4160] * 7

LISTS = {"A": A, "B": B, "C": C, "D": D, "D1": D1, "E": E, "F1": F1, "F2": F2}


def offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def shard(buf, per, sizes, b, j):
    """Shard j of block b in a flat ragged buffer of `per` shards per block:
    bytes [per * off[b] + j * S[b], + S[b])."""
    off = offsets(sizes)
    lo = per * off[b] + j * sizes[b]
    return buf[lo:lo + sizes[b]]
