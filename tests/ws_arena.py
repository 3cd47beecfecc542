"""A poisoned, guarded arena for the caller workspaces of the C ABI: the instrument of tests/test_gpu_workspace.py and
tests/test_workspace_host.py (a helper module: no conftest, and nothing in the package imports it).

Every compute entry with a ``(void* ws, size_t bytes)`` pair is sized by its own ``mm_*_workspace_bytes*`` function, and the
wrappers allocate that many bytes with torch.empty: the caching allocator rounds the request up, hands the slack to nobody
or to a neighbour, and returns memory that is zero or holds the previous call's values.  So a sizer that is a row short, a
launch that reads a word it never set and a write in front of the workspace all pass.  Here the entry gets EXACTLY the
bytes its sizer named, in the middle of memory the test owns:

    [ guard 256 KiB | nbytes, rounded up to 256 | guard 256 KiB ]      every byte = fill

``Arena.ws`` is the view [guard, guard + nbytes): data_ptr() and numel() are what the entry sees, at torch's own base
alignment (the guard is a multiple of 256).  The slack of the round-up behind nbytes counts as guard.  256 KiB is above
any row or plane of the registry's shapes; a stray write farther away than that is outside what a guard can show.

The patterns: 0x00, what a fresh allocation usually holds; 0xFF, NaN in floats and -1 in integers; 0x7F, about 3.39e38 in
float32, 1.4e306 in float64 and an int32 of 2139062143 that wins every atomicMax against the key of a finite float.  Both
non-zero patterns are needed: a NaN loses in v_max and -1 loses in atomicMax, so only 0x7F shows an unset clip key and only
0xFF a float that leaked into a sum.
"""
from __future__ import annotations

GUARD = 256 * 1024
PATTERNS = (0x00, 0xFF, 0x7F)


def _round_up(n, m):
    return (int(n) + m - 1) // m * m


class Arena:
    def __init__(self, nbytes, device, fill):
        import torch
        nbytes = int(nbytes)
        assert nbytes >= 0 and 0 <= fill <= 0xFF and GUARD % 256 == 0
        self.nbytes, self.fill = nbytes, int(fill)
        self.base = torch.empty(GUARD + _round_up(nbytes, 256) + GUARD, dtype=torch.uint8, device=device)
        self.refill()
        self.ws = self.base[GUARD:GUARD + nbytes]
        assert self.ws.numel() == nbytes and (nbytes == 0 or self.ws.data_ptr() == self.base.data_ptr() + GUARD)

    def refill(self):
        """The pattern over the whole arena, workspace included (a torch op on the current stream)."""
        self.base.fill_(self.fill)

    def altered(self):
        """None, or the first altered guard byte as (side, offset): ("front", -k) is k bytes in front of the workspace's
        first byte, ("back", +k) is k bytes behind its end (+0: the byte at ws[nbytes])."""
        front, back = self.base[:GUARD], self.base[GUARD + self.nbytes:]
        for side, region in (("front", front), ("back", back)):
            bad = region != self.fill
            if bool(bad.any()):
                i = int(bad.nonzero()[0])
                return (side, i - GUARD) if side == "front" else (side, i)
        return None

    def check(self, what=""):
        hit = self.altered()
        if hit is not None:
            side, off = hit
            where = f"{-off} bytes in front of the workspace's start" if side == "front" else f"{off} bytes past the workspace's end"
            raise AssertionError(f"{what}: a guard byte of a {self.nbytes}-byte workspace (fill 0x{self.fill:02X}) was altered: the "
                                 f"first one lies {where} (offset {off:+d} from its {'start' if side == 'front' else 'end'})")


class Arenas:
    """Hands arenas out and keeps every base tensor alive until close(): a wrapper drops its ``ws`` right after the call,
    and the memory must stay ours until it has been checked.  ``sized`` is the log of the sizer calls redirect() saw."""

    def __init__(self, device, fill):
        self.device, self.fill = device, fill
        self.all = []
        self.sized = []          # (sizer name, bytes) of every *_workspace_bytes* call made while redirected

    def get(self, nbytes, device=None):
        a = Arena(nbytes, self.device if device is None else device, self.fill)
        self.all.append(a)
        return a.ws

    def of(self, ws):
        """The arena a handed-out workspace lies in."""
        for a in self.all:
            if a.ws is ws:
                return a
        raise KeyError("not a workspace of these arenas")

    @property
    def count(self):
        return len(self.all)

    @property
    def sizes(self):
        return [a.nbytes for a in self.all]

    def refill(self):
        for a in self.all:
            a.refill()

    def check(self, what=""):
        for i, a in enumerate(self.all):
            a.check(f"{what}: arena {i} of {len(self.all)}")

    def check_handed_out(self, what=""):
        """The hand-out condition: a call whose sizer named a positive size took its scratch from here (a wrapper that
        allocates past the redirect is not under test at all), and every arena is exactly as large as a sizer said."""
        positive = sorted({(n, v) for n, v in self.sized if v > 0})
        assert not (positive and not self.all), f"{what}: {positive} but no workspace was taken from the arenas"
        if self.sized:
            named = {v for _, v in self.sized}
            odd = [s for s in self.sizes if s not in named]
            assert not odd, f"{what}: workspaces of {odd} bytes, the sizers named {sorted(named)}"

    def close(self):
        self.all.clear()


def redirect(monkeypatch, arenas):
    """Points the three allocation sites at ``arenas``: modulation_mfcc_amd._lib.workspace, MfccPlan.workspace /
    MfccPlan.ragged_workspace (the sizer calls of plan.py; an arena of exactly ``need`` bytes on every call, not the plan's
    cached buffer) and stream_cases.Prepared.work; and logs every *_workspace_bytes* call of the loaded library in
    ``arenas.sized``.  The wrappers use nothing of a workspace but data_ptr() and numel()."""
    import stream_cases as S
    from modulation_mfcc_amd import _lib as L
    from modulation_mfcc_amd.plan import MfccPlan

    monkeypatch.setattr(L, "workspace", lambda nbytes, dev: arenas.get(nbytes, dev))

    def workspace(self, batch, n_samples):
        need = int(self._lib.mm_workspace_bytes(self._h, batch, n_samples))
        return arenas.get(need, self.device)

    def ragged_workspace(self, batch, n_samples):
        need = int(self._lib.mm_ragged_workspace_bytes(self._h, batch, n_samples))
        if need == 0:
            raise ValueError("mm_ragged_workspace_bytes: invalid arguments")
        return arenas.get(need, self.device)

    monkeypatch.setattr(MfccPlan, "workspace", workspace)
    monkeypatch.setattr(MfccPlan, "ragged_workspace", ragged_workspace)
    monkeypatch.setattr(S.Prepared, "work", lambda self, nbytes: arenas.get(nbytes, self.gpu))

    lib = L.load()
    for name in sizer_names():
        def logged(*a, _fn=getattr(lib, name), _name=name):
            v = int(_fn(*a))
            arenas.sized.append((_name, v))
            return v
        monkeypatch.setattr(lib, name, logged)


def tables():
    from modulation_mfcc_amd import _lib as L
    return (L.PROTOTYPES, L.PROTOTYPES_MODPSD, L.PROTOTYPES_MODCSD, L.PROTOTYPES_SPLINE, L.PROTOTYPES_LOMB, L.PROTOTYPES_ZOOM)


def sizer_names():
    """Every *_workspace_bytes* symbol of the ctypes tables."""
    return [n for t in tables() for n in t if "_workspace_bytes" in n]
