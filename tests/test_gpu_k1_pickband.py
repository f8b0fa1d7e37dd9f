"""The draw kernel's quad on the device (msim_pipeline.h k1p_quad_fast: the picker by one multiply with 400,
msim_fastdraw.h pick_off400_key) from start states crafted around the picker's band, in both instantiations,
against the oracle's NextBlockInterval and PickFinder stepped from the same states.

With 400 h' = t 2^32 + L the quad takes the exact path when L >= 2^32 - 1024. The picker stream is crafted so that
its high-word output h' lands, at each of the four quad positions and with and without a carry out of the low
halves (the true high word is then h' + 1): just inside the band, just below it, in the band with t mod 4 != 3
(where the multiply with 100 did not flag), at the wrap h' = 2^32 - 1, and at PickFinder's fall-through (the top
sixteen draws, index 100). The interval stream carries u = 0, u = 2^64 - 1 and draws with v < 2^-15 beside them."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 31_556_952_000
H = [30, 29, 12, 11, 8, 5, 3, 1, 1]
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
BAND = (1 << 32) - 1024


def _rotl(x, k):
    return ((x << k) | (x >> (64 - k))) & M64


def _next(s):  # xoroshiro128++: (output, next state)
    s0, s1 = s
    out = (_rotl((s0 + s1) & M64, 17) + s0) & M64
    s1 ^= s0
    return out, ((_rotl(s0, 49) ^ s1 ^ ((s1 << 21) & M64)) & M64, _rotl(s1, 28))


def _back(s):  # the state before s
    t = _rotl(s[1], 36)
    x = s[0] ^ t ^ ((t << 21) & M64)
    s0 = _rotl(x, 15)
    return (s0, t ^ s0)


def _start_for(u, pos, s0):
    """A start state whose draw number pos (0-3) is u, with the given s0 at that draw."""
    x = (u - s0) & M64
    s = (s0, (_rotl(x, 47) - s0) & M64)
    for _ in range(pos):
        s = _back(s)
    return s


def _picker_targets():
    """(kind, h', carry, low word): the draw is ((h' + carry) mod 2^32, low)."""
    inv25 = pow(25, -1, 1 << 28)
    out = []
    for kind, lows in (("inside", [BAND, BAND + 16, BAND + 512, (1 << 32) - 32, (1 << 32) - 16]),
                       ("below", [BAND - 16, BAND - 32, BAND - 1024])):
        for L in lows:  # 400 h' = L (mod 2^32): h' = (L / 16) / 25 (mod 2^28), any top four bits
            for top in range(16):
                hp = ((L // 16) * inv25 % (1 << 28)) | (top << 28)
                assert (400 * hp) & M32 == L
                j = ((400 * hp) >> 32) & 3
                for carry in (0, 1):
                    out.append((kind if kind == "below" or j == 3 else "inside_j", hp, carry, 0 if carry else M32))
    out.append(("wrap", M32, 1, 0))       # the true high word is 0: index 0, where p(h') = 99
    out.append(("wrap", M32, 1, 12345))
    out.append(("wrap", M32, 0, 0))       # index 99
    for low in range(M32 - 16, M32 + 1):  # the last draw of index 99, then index 100: PickFinder falls through
        out.append(("fall", M32, 0, low))
    out.append(("fall", M32 - 1, 1, M32 - 5))  # index 100 reached through a carry
    return out


def _interval_targets():
    top = M64 - (1 << 49)  # v = 1 - (u >> 11) 2^-53 < 2^-15 from here up
    return [0, M64, top + 1, M64 - (1 << 11), M64 - (1 << 30), 1 << 11, top + (1 << 40)]


@pytest.fixture(scope="module")
def quads(oracle):
    """Start states and the oracle's four intervals and four finders (15: fell through) for the network H."""
    rng = np.random.default_rng(20240)
    L = oracle.lib()
    perc = (ctypes.c_uint64 * len(H))(*H)
    iu = _interval_targets()
    states, want, kinds = [], [], []
    n = 0
    for kind, hp, carry, low in _picker_targets():
        for pos in range(4):
            for rep in range(3):
                # the low halves carry iff u_lo < s0_lo
                s0 = int(rng.integers(0, 1 << 63)) << 1
                if carry:
                    s0 = (s0 & ~M32) | max(low + 1, int(rng.integers(low + 1, 1 << 32)))
                else:
                    s0 = (s0 & ~M32) | int(rng.integers(0, low + 1))
                up = (((hp + carry) & M32) << 32) | low
                rp = _start_for(up, pos, s0)
                ui = iu[n % len(iu)]
                posi = (n // len(iu)) % 4
                ri = _start_for(ui, posi, int(rng.integers(0, 1 << 63)) << 1 | 1)
                # the crafting itself: the draws at the positions, and the high-word output step's h'
                s, t = rp, ri
                for q in range(4):
                    if q == pos:
                        hprime = ((_rotl((s[0] + s[1]) & M64, 17) >> 32) + (s[0] >> 32)) & M32
                        assert hprime == hp, (kind, hp, carry, low)
                    o, s = _next(s)
                    assert q != pos or o == up
                    o, t = _next(t)
                    assert q != posi or o == ui
                a, b = oracle.ORng(*ri), oracle.ORng(*rp)
                row = [L.oracle_next_block_interval(ctypes.byref(a)) for _ in range(4)]
                row += [L.oracle_pick_finder(perc, len(H), ctypes.byref(b)) & 15 for _ in range(4)]  # -1 -> 15
                states.append(ri + rp)
                want.append(row)
                kinds.append((kind, pos))
                n += 1
    states = np.array(states, dtype=np.uint64)
    want = np.array(want, dtype=np.int64).astype(np.uint32)
    assert 2_000 < states.shape[0] < 6_000
    for kind in ("inside", "inside_j", "below", "wrap", "fall"):
        for pos in range(4):
            assert (kind, pos) in kinds
    assert (want[:, 4:] == 15).any(axis=0).all()  # the fall-through at every position
    assert (want[:, :4] == 0).any() and (want[:, :4] > 6_000_000).any()  # u = 0; v < 2^-15: over 6e5 * 15 ln 2 ms
    return states, want


@pytest.mark.parametrize("name,props", [
    ("uniform", [100] * 9),                                                  # msim_draws_kernel<true>'s form
    ("per_finder", [100, 100, 100, 1000, 1000, 1000, 10_000, 10_000, 0]),    # <false>'s
])
def test_gpu_k1_pickband(msim_lib_path, quads, name, props):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.set_device(0)
    import miningsimulation_amd as msim
    from miningsimulation_amd import _lib

    states, want = quads
    n = states.shape[0]
    sim = msim.Simulation([msim.Miner(k, H[k], props[k], False) for k in range(len(H))], D)
    fn = _lib.lib.msim_device_k1_quads
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    ds = torch.from_numpy(states.view(np.int64).copy()).cuda()
    do = torch.full((n, 8), -1, dtype=torch.int32, device="cuda")
    _lib.check(fn(sim.handle, ctypes.c_void_p(ds.data_ptr()), ctypes.c_void_p(do.data_ptr()), n, None))
    torch.cuda.synchronize()
    got = do.cpu().numpy().view(np.uint32)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (name, bad[:8], states[bad[:8]], want[bad[:8]], got[bad[:8]])
