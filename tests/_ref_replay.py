"""Recorded answers of the reference's own kernels compiled for the CPU (oracle/_ref) to the calls of tests/test_oracle_vs_reference.py, so that
the pin against the reference holds where oracle/_ref cannot be built (no reference sources on the machine): tests/golden/ref_calls_<i>.npz.

Every call is keyed by a digest of the method name and its inputs.  Recording (tests/golden/make_ref_calls.py) makes the same call on the C
oracle as well: an output of the reference that is large and bit for bit the oracle's is stored as the SHA-256 of its bytes, every other output
in full (returned arrays, and the arrays the call updated in place).  Replay makes the call on the oracle and hands back, for a digest-only
output, the oracle's array once its digest matches the recorded one (the reference's bytes, as the digest proves) -- else it fails the test,
which is what the bit-exact assertions on these outputs would do against the live reference -- and the stored array for every other output.
The recording is split by call key over SHARDS files, ref_calls_<i>.npz, each below 1 MiB."""
import glob
import hashlib
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHARDS = 4
DIGEST_ONLY_BYTES = 1 << 16        # outputs at least this large that equal the oracle's bit for bit are stored as a digest


def _sha(a: np.ndarray) -> str:
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes()).hexdigest()


def call_key(name, args, kwargs) -> str:
    h = hashlib.sha256(name.encode())
    for v in list(args) + [kwargs[k] for k in sorted(kwargs)] + sorted(kwargs):
        h.update(_sha(v).encode() if isinstance(v, np.ndarray) else repr(v).encode())
    return h.hexdigest()[:24]


def _copy(args, kwargs):
    return ([a.copy() if isinstance(a, np.ndarray) else a for a in args],
            {k: v.copy() if isinstance(v, np.ndarray) else v for k, v in kwargs.items()})


def _arrays(args, kwargs):
    """the array arguments by position: 'a<i>' / 'k<name>'"""
    out = {f"a{i}": a for i, a in enumerate(args) if isinstance(a, np.ndarray)}
    out.update({f"k{k}": v for k, v in kwargs.items() if isinstance(v, np.ndarray)})
    return out


def _returns(r):
    return (list(r), True) if isinstance(r, tuple) else ([r], False)


class Recorder:
    """wraps the live reference ops; every call is answered by the reference and recorded next to the oracle's answer"""

    def __init__(self, ref, orc):
        self._ref, self._orc, self.store = ref, orc, {}

    def __getattr__(self, name):
        def call(*args, **kwargs):
            key = call_key(name, args, kwargs)
            o_args, o_kwargs = _copy(args, kwargs)
            before = {k: v.copy() for k, v in _arrays(args, kwargs).items()}
            got, tup = _returns(getattr(self._ref, name)(*args, **kwargs))
            mine, _ = _returns(getattr(self._orc, name)(*o_args, **o_kwargs))
            outs = {f"r{i}": (g, m) for i, (g, m) in enumerate(zip(got, mine))}
            o_arr = _arrays(o_args, o_kwargs)
            outs.update({k: (v, o_arr[k]) for k, v in _arrays(args, kwargs).items() if not np.array_equal(v, before[k], equal_nan=True)})
            self.store[f"{key}/meta"] = np.array([len(got), int(tup)], np.int64)
            for slot, (g, m) in outs.items():
                if g is None:                                          # (composite_rays answers in place)
                    self.store[f"{key}/{slot}/none"] = np.zeros(0, np.int8)
                    continue
                g = np.asarray(g)
                if g.nbytes >= DIGEST_ONLY_BYTES and g.shape == np.shape(m) and np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(m).tobytes():
                    self.store[f"{key}/{slot}/sha"] = np.array(_sha(g))
                else:
                    self.store[f"{key}/{slot}"] = g
            return tuple(got) if tup else got[0]
        return call

    def save(self, golden=GOLDEN):
        for f in glob.glob(os.path.join(golden, "ref_calls_*.npz")):
            os.remove(f)
        for i in range(SHARDS):
            np.savez_compressed(os.path.join(golden, f"ref_calls_{i}.npz"), **{k: v for k, v in self.store.items() if int(k[:8], 16) % SHARDS == i})


class Replay:
    """answers the calls from the recording, with the oracle computing the outputs that were recorded as digests"""

    def __init__(self, orc, golden=GOLDEN):
        self._orc, self._z = orc, {}
        for i in range(SHARDS):
            with np.load(os.path.join(golden, f"ref_calls_{i}.npz")) as z:
                self._z.update({k: z[k] for k in z.files})

    def __getattr__(self, name):
        def call(*args, **kwargs):
            import pytest
            key = call_key(name, args, kwargs)
            if f"{key}/meta" not in self._z:
                pytest.fail(f"ref.{name}: no recorded reference answer for these inputs (tests/golden/make_ref_calls.py records them)")
            n_ret, tup = (int(x) for x in self._z[f"{key}/meta"])
            o_args, o_kwargs = _copy(args, kwargs)
            mine, _ = _returns(getattr(self._orc, name)(*o_args, **o_kwargs))
            o_arr = _arrays(o_args, o_kwargs)

            def answer(slot, oracle_value):
                if f"{key}/{slot}/none" in self._z:
                    return None
                if f"{key}/{slot}" in self._z:
                    return self._z[f"{key}/{slot}"].copy()
                want = str(self._z[f"{key}/{slot}/sha"])
                if _sha(np.asarray(oracle_value)) != want:
                    pytest.fail(f"ref.{name} output {slot}: the oracle no longer reproduces the reference's recorded bytes")
                return np.asarray(oracle_value).copy()

            got = [answer(f"r{i}", mine[i]) for i in range(n_ret)]
            for slot, arr in _arrays(args, kwargs).items():            # arrays the reference updated in place
                if f"{key}/{slot}" in self._z or f"{key}/{slot}/sha" in self._z:
                    np.copyto(arr, answer(slot, o_arr[slot]))
            return tuple(got) if tup else got[0]
        return call
