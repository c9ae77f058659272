"""The random stream of a seeded request (include/ssd_hip_seed.h), restated in numpy uint64 / float32:

    key(seed, purpose, pos)    = mix64( mix64(seed) ^ (purpose << 56) ^ pos )
    u(seed, purpose, pos, idx) = (float32(mix64(key ^ idx) >> 40) + 0.5) * 2^-24

Everything broadcasts; 64-bit arithmetic wraps."""
import numpy as np

DRAFT, TARGET, ACCEPT = 1, 2, 3

_U = np.uint64


def mix64(z):
    z = np.asarray(z, dtype=_U)
    with np.errstate(over="ignore"):
        z = z + _U(0x9e3779b97f4a7c15)
        z = (z ^ (z >> _U(30))) * _U(0xbf58476d1ce4e5b9)
        z = (z ^ (z >> _U(27))) * _U(0x94d049bb133111eb)
    return z ^ (z >> _U(31))


def key(seed, purpose, pos):
    """pos: the absolute position of the token being decided (the kernels take the input token's position and add 1)."""
    return mix64(mix64(seed) ^ (np.asarray(purpose, dtype=_U) << _U(56)) ^ np.asarray(pos, dtype=_U))


def bits24(seed, purpose, pos, idx):
    return mix64(key(seed, purpose, pos) ^ np.asarray(idx, dtype=_U)) >> _U(40)


def uniform(seed, purpose, pos, idx):
    """float32, the device's value by bits: the conversion of a 24-bit integer is exact, the + 0.5 rounds to nearest-even in float32
    on both sides (it is inexact from 2^23 on), and the scale is a power of two."""
    return (bits24(seed, purpose, pos, idx).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
