"""Exact-size, poisoned, guarded scratch for every launch that goes through ``ops._workspace`` (test infrastructure).

The C ABI (include/contrad_hip.h) lets the caller allocate every workspace: exactly ``*_workspace_bytes`` bytes, 16-byte
aligned, contents undefined.  The Python wrappers take theirs from ``ops._workspace``, a grow-only cache that is almost always
larger than the request, 512-byte aligned, and still holds what the previous launch left.  ``WorkspaceGuard`` replaces that
function while it is active (the wrappers look the name up at call time) and hands every request storage of its own:

    [ front guard | nbytes rounded up to 4 | back guard ]          all of it filled with one 32-bit poison word

The float32 view that is returned starts 16-byte aligned and deliberately NOT 32-byte aligned (the front guard is an odd
multiple of 16 bytes behind a 32-byte aligned start), and the back guard begins at its last byte + 1.  Every buffer stays
alive until ``check()``, which synchronises once and asserts that both guards of every request still hold the poison word.

    with WorkspaceGuard(POISONS['qnan']) as g:
        y = ops.conv2d_fwd(...)
        g.check()
    assert g.log[0].nbytes == expected

With a NaN poison an unwritten workspace element that reaches an output makes that output NaN, and so does a read past the
end that reaches one; a write outside [workspace, workspace + nbytes) breaks a guard (within FRONT_BYTES / BACK_BYTES of it).
"""
import sys

import torch

from contrad_amd import ops

POISONS = {
    'qnan': 0x7fc00000,         # a quiet NaN
    'ones': 0xffffffff,         # a NaN as a float, -1 as an int, the maximum as an unsigned, a NaN as either half of a double
    'zero': 0x00000000,
}

FRONT_BYTES = 16 * 65           # an odd multiple of 16
BACK_BYTES = 4096
_ALIGN = 32


def _as_i32(word):
    return word - (1 << 32) if word >= (1 << 31) else word


class GuardError(AssertionError):
    pass


class Request(object):
    __slots__ = ('index', 'nbytes', 'caller', 'raw', 'front', 'view', 'back')

    def __repr__(self):
        return 'workspace request #%d (%d bytes, from ops.%s)' % (self.index, self.nbytes, self.caller)


class WorkspaceGuard(object):
    def __init__(self, poison):
        self.poison = int(poison)
        self.log = []
        self._saved = None

    # -- patching ------------------------------------------------------------------------------------------------------
    def __enter__(self):
        self._saved = ops._workspace
        ops._workspace = self._request
        return self

    def __exit__(self, *exc):
        ops._workspace = self._saved
        self._saved = None
        return False

    # -- the replacement of ops._workspace -----------------------------------------------------------------------------
    def _request(self, nbytes, device):
        n = (max(int(nbytes), 1) + 3) // 4 * 4                      # as ops._workspace rounds
        raw = torch.empty(FRONT_BYTES + n + BACK_BYTES + _ALIGN, dtype=torch.uint8, device=device)
        start = -raw.data_ptr() % _ALIGN                            # a 32-byte aligned start inside the allocation
        body = raw[start:start + FRONT_BYTES + n + BACK_BYTES]
        body.view(torch.int32).fill_(_as_i32(self.poison))
        r = Request()
        r.index, r.nbytes, r.raw = len(self.log), int(nbytes), raw
        f = sys._getframe(1)
        names = [f.f_code.co_name]
        while names[-1].startswith('_') and f.f_back is not None:   # a private helper: name the wrapper that called it too
            f = f.f_back
            names.append(f.f_code.co_name)
        r.caller = ' <- '.join(names)
        r.front = body[:FRONT_BYTES].view(torch.int32)
        r.view = body[FRONT_BYTES:FRONT_BYTES + n].view(torch.float32)
        r.back = body[FRONT_BYTES + n:].view(torch.int32)
        assert r.view.data_ptr() % 32 == 16
        self.log.append(r)
        return r.view

    # -- the check -----------------------------------------------------------------------------------------------------
    def check(self):
        """Synchronise once, then assert that both guards of every request still hold the poison word."""
        if any(r.raw.is_cuda for r in self.log):
            torch.cuda.synchronize()
        if not self.log:
            return
        word = _as_i32(self.poison)
        bad = torch.stack([torch.stack([(r.front != word).sum(), (r.back != word).sum()]) for r in self.log]).cpu()
        problems = []
        for r, (nf, nb) in zip(self.log, bad.tolist()):
            for side, guard, cnt in (('front', r.front, nf), ('back', r.back, nb)):
                if cnt:
                    first = int((guard != word).nonzero()[0])
                    at = 4 * first - FRONT_BYTES if side == 'front' else r.view.numel() * 4 + 4 * first
                    problems.append('%r: %s guard overwritten (%d words, first at byte offset %d from the workspace base, '
                                    'holds 0x%08x)' % (r, side, cnt, at, int(guard[first]) & 0xffffffff))
        if problems:
            raise GuardError('; '.join(problems))

    def requests(self, caller=None):
        return [r for r in self.log if caller is None or caller in r.caller.split(' <- ')]
