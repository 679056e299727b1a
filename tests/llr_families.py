"""Fixed-point LLR input families: plain numpy transforms of an AWGN flow array [..., 3K+12]
(pyoracle.synth_batch / make_frames).  A receiver hands the decoder multiples of a quantum,
saturated, with exact zeros at punctured positions; on such input the max* differences sit exactly
on bucket edges, hard decisions tie at LLR == 0, and the exact log-MAP kernel's speculation detector
fires (oracle/turbo_oracle_spec.inc).  Every output value is exactly representable in fp32 (at most
8 significant bits), so casting a family to float32 changes nothing.

int8_q16 is int8 carried as raw Q16 integers (x 65536, |LLR| up to 8.3e6).  On the narrow families a
speculation miss sits beside a bucket edge, where the speculated and the exact table row give the
same correction, so the kernel's recomputation changes no value; at this magnitude fp32 roundings of
the metrics reach the distance between a bucket edge and the threshold inside the bucket, the two
rows give different corrections, and only the recomputation keeps the decode exact
(pyoracle.spec_miss_turbo's harmful count)."""
import numpy as np


def q4(f):
    return np.clip(np.round(4.0 * f) / 4.0, -8.0, 8.0)


def q8(f):
    return np.clip(np.round(8.0 * f) / 8.0, -16.0, 16.0)


def int31(f):
    return np.clip(np.round(2.0 * f), -31.0, 31.0)


def int8(f):
    return np.clip(np.round(16.0 * f), -127.0, 127.0)


def int8_q16(f):
    return int8(f) * 65536.0


def sign(f):
    return np.sign(f)


def zero(f):
    return np.zeros_like(f)


def punct(f):
    """Every second parity value of each parity stream set to 0.0 (the stream of 3K+12: triples
    (systematic, parity 1, parity 2) for K positions, then the 12 tail values, left alone)."""
    f = np.array(f, dtype=np.float64, copy=True)
    K = (f.shape[-1] - 12) // 3
    body = f[..., :3 * K].reshape(f.shape[:-1] + (K, 3))
    body[..., 1::2, 1] = 0.0
    body[..., 1::2, 2] = 0.0
    return f


FAMILIES = {"q4": q4, "q8": q8, "int31": int31, "int8": int8, "int8_q16": int8_q16, "sign": sign, "zero": zero, "punct": punct}


def apply(name, flow):
    """The family `name` of flow, float64, contiguous and read-only."""
    out = np.ascontiguousarray(FAMILIES[name](np.asarray(flow, dtype=np.float64)), dtype=np.float64)
    out.setflags(write=False)
    return out
