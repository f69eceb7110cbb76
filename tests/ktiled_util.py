"""The k-step-tiled copy of a row-major bf16 B[N][K], restated in numpy straight from its definition
(include/ptk.h, ptk_kstep_tile_offset): block (g, s) holds rows 16g .. 16g + 15 of k elements 32s .. 32s + 31 at
byte (g * (K / 32) + s) * 1024; its 16-byte unit i holds row 16g + (i >> 2), 16-byte k-chunk (i & 3) ^ ((i >> 3) & 2)."""
import numpy as np


def tiled_source_index(N, K):
    """src[j] = flat row-major element index (row * K + k) stored at element j of the tiled copy."""
    assert N % 16 == 0 and K % 32 == 0
    ks = K // 32
    g, s, i, e = np.meshgrid(np.arange(N // 16), np.arange(ks), np.arange(64), np.arange(8), indexing="ij")
    row = 16 * g + (i >> 2)
    chunk = (i & 3) ^ ((i >> 3) & 2)
    k = 32 * s + 8 * chunk + e
    return (row * K + k).reshape(-1).astype(np.int64)   # (g, s, i, e) in storage order: 1024 B, 16 B, 2 B strides
