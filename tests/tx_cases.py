"""Shared by the modulator tests (test_tx_ref_cpu, test_tx_cpu, test_tx_gpu)
and tests/golden/make_tx_golden.py: the float64 numpy statement of
ofdm_tx_modulate's semantics (include/ofdm_lsmrc.h), the seeded inputs, the
fixture files and the build of the reference harness."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-accel-ofdm-ls-mrc_amd")
GOLDEN_TX = os.path.join(ROOT, "tests", "golden", "tx")
PILOTS = os.path.join(ROOT, "tests", "golden", "Pilots.dat")
REF = os.environ.get("REF", "/root/reference")

# (rows, C, prefix) of the recorded reference runs, and the seed of each
REF_SHAPES = [(3, 1024, 0), (2, 1024, 16), (2, 64, 4), (2, 9, 2)]
REF_FUNCS = ["matrix_readX", "ifftShiftOneRow", "ifftOneRow", "addPrefix", "multiplyWithChannelInv",
             "modRefSymbol", "modOneSymbol"]


def seed_of(rows, C, prefix):
    return 7000 + 100 * rows + C + 31 * prefix


def fixture_path(rows, C, prefix):
    return os.path.join(GOLDEN_TX, f"tx_r{rows}_c{C}_p{prefix}.npz")


def rows_of(seed, rows, K):
    """Seeded complex64 rows, CN(0, 1)."""
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((rows, K)) + 1j * rng.standard_normal((rows, K))) * np.sqrt(0.5)).astype(np.complex64)


# ------------------------------------------------------- float64 statement

def out_src(k, K):
    """common.hpp out_src: the subcarrier shiftOneRow's memmoves put at output position k."""
    h, n2 = (K - 1) // 2, (K + 1) // 2
    return k + h if k < n2 else (k - n2 if k < n2 + h else k)


def out_pos_any(j, K):
    """common.hpp out_pos_any, the inverse of out_src; also matrix_readX's
    memmoves (cpuLS.hpp:105-112): rotated[j] = raw[out_pos_any(j, K)]."""
    h, n2 = (K - 1) // 2, (K + 1) // 2
    return j + n2 if j < h else (j - h if j < h + n2 else j)


def bin_of(k, C, map):
    """The transform bin that carries input position k."""
    if map == "reference":  # d[k + 1] = X[k], then ifftShiftOneRow's memmoves with h = C // 2
        h, i = C // 2, k + 1
        return i - h if h <= i < 2 * h else (i + h if i < h else i)
    return out_src(k, C - 1) + 1


def tx_bins(X, C, map):
    X = np.asarray(X, np.complex128)
    bins = np.zeros(X.shape[:-1] + (C,), np.complex128)
    for k in range(C - 1):
        bins[..., bin_of(k, C, map)] = X[..., k]
    return bins


def tx_numpy(X, C, cp=0, map="rx", norm="scale", scale=1.0):
    """(iq (..., C + cp) complex128, peak (...,) float64) of rows X (..., >= K); only the first K columns are read."""
    x = np.fft.ifft(tx_bins(np.asarray(X)[..., :C - 1], C, map), axis=-1) * C  # backward, unnormalised
    peak = np.abs(x).max(axis=-1)
    with np.errstate(divide="ignore"):
        g = np.where(peak > 0, 1.0 / peak, 0.0) if norm == "peak" else np.full(peak.shape, float(scale))
    y = x * g[..., None]
    return np.concatenate([y[..., C - cp:], y], axis=-1), peak


# ---------------------------------------------------- the reference's code

def reference_present():
    return os.path.exists(os.path.join(REF, "cpuLS.hpp"))


def build_ref_harness(tmp, prefix):
    """The reference's transmit functions, read where they lie (from each
    definition line to the first closing brace in column 0, as
    oracle/build_ref.sh does), behind tests/cpp/tx_ref_standins.hpp and in
    front of tests/cpp/tx_ref_harness.cpp -> a shared library in tmp."""
    src = open(os.path.join(REF, "cpuLS.hpp"), errors="replace").read().splitlines()
    text = []
    for fn in REF_FUNCS:
        on = False
        for ln in src:
            if ln.startswith(f"void {fn}("):
                on = True
            if on:
                text.append(ln)
                if ln.startswith("}"):
                    break
        assert on, f"{fn} not found in the reference"
    text.append(open(os.path.join(ROOT, "tests", "cpp", "tx_ref_harness.cpp")).read())
    so = os.path.join(str(tmp), f"libtx_ref_p{prefix}.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-DHAVE_UNISTD_H=1", f"-Dprefix={prefix}",
                    f"-I{REF}", "-include", os.path.join(ROOT, "tests", "cpp", "tx_ref_standins.hpp"),
                    "-x", "c++", "-", "-o", so], input="\n".join(text).encode(), check=True)
    return so


class RefTx:
    def __init__(self, tmp, prefix):
        self.prefix = prefix
        self.L = ctypes.CDLL(build_ref_harness(tmp, prefix))
        assert self.L.tx_ref_prefix() == prefix

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    def ifftshift(self, d):
        y = np.ascontiguousarray(d, np.complex64).copy()
        self.L.tx_ref_ifftshift(self._p(y), y.size)
        return y

    def ifft(self, d):
        y = np.ascontiguousarray(d, np.complex64).copy()
        self.L.tx_ref_ifft(self._p(y), y.size)
        return y

    def add_prefix(self, dY):
        dY = np.ascontiguousarray(dY, np.complex64)
        rows, cols = dY.shape
        Y = np.zeros((rows, cols + self.prefix), np.complex64)
        self.L.tx_ref_add_prefix(self._p(Y), self._p(dY), rows, cols)
        return Y

    def mod_ref_symbol(self, C, path=PILOTS):
        Y = np.zeros(C + self.prefix, np.complex64)
        X = np.zeros(C - 1, np.complex64)
        self.L.tx_ref_mod_ref_symbol(self._p(Y), self._p(X), C, path.encode())
        return Y, X

    def mod_one_symbol(self, X, C):
        X = np.ascontiguousarray(X, np.complex64).copy()
        users = X.shape[0]
        assert X.shape == (users, C - 1)
        Y = np.zeros((users, C + self.prefix), np.complex64)
        self.L.tx_ref_mod_one_symbol(self._p(Y), self._p(X), C, users)
        return Y


def build_tx_driver(tmp, prefix):
    """tests/cpp/tx_driver.cpp against the drop-in cpuLS.hpp + the library, for one prefix length."""
    exe = os.path.join(str(tmp), f"tx_driver_p{prefix}")
    subprocess.run(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", f"-Dprefix={prefix}", "-I/opt/rocm/include",
                    f"-I{PKG}/host", f"-I{ROOT}/include", os.path.join(ROOT, "tests", "cpp", "tx_driver.cpp"),
                    "-o", exe, f"-L{PKG}/lib", "-lofdm_lsmrc", f"-Wl,-rpath,{PKG}/lib",
                    "-L/opt/rocm/lib", "-lamdhip64", "-lrt"], check=True)
    return exe


def reference_record(tmp, rows, C, prefix):
    """What one fixture holds: the seeded rows through the reference's
    modOneSymbol, and its modRefSymbol on tests/golden/Pilots.dat."""
    ref = RefTx(tmp, prefix)
    seed = seed_of(rows, C, prefix)
    X = rows_of(seed, rows, C - 1)
    ref_iq, ref_X = ref.mod_ref_symbol(C)
    return dict(domain=np.array("tx"), seed=np.int64(seed), rows=np.int64(rows), C=np.int64(C),
                prefix=np.int64(prefix), X=X, iq=ref.mod_one_symbol(X, C), ref_X=ref_X, ref_iq=ref_iq)


def load_fixture(rows, C, prefix):
    return np.load(fixture_path(rows, C, prefix), allow_pickle=False)
