"""The numpy full-matrix Smith-Waterman of the gapped-stage tests (tests/test_sw_kernels.py, tests/test_matrix_cases.py): an independent restatement
of the recurrence and of the orientation S[query letter][target letter]."""
import numpy as np


class Dp:
    """full-matrix integer Smith-Waterman (affine gaps, open >= extension) in numpy: every H, for the questions the oracle's end cell
    cannot answer - is the end row ambiguous, does one row hold every optimal cell"""

    def __init__(self, p):
        self.S3 = np.array(p.S3[:], np.int32).reshape(21, 21)
        self.SA = np.array(p.SA[:], np.int32).reshape(21, 21)
        self.open, self.ext = p.gap_open, p.gap_ext
        assert self.open >= self.ext >= 0          # E from the row's H before its own gaps is exact then

    def H(self, q3, qa, t3, ta):
        S = self.S3[q3][:, t3] + self.SA[qa][:, ta]
        lq, lt = S.shape
        H = np.zeros((lq, lt), np.int32)
        hp, fp = np.zeros(lt + 1, np.int32), np.full(lt + 1, -(1 << 28), np.int32)
        ar = np.arange(lt + 1, dtype=np.int32) * self.ext
        for i in range(lq):
            f = np.maximum(fp - self.ext, hp - self.open)
            h = np.maximum(np.maximum(hp[:-1] + S[i], f[1:]), 0)
            m = np.maximum.accumulate(np.concatenate(([0], h)) + ar)
            h = np.maximum(h, m[:-1] - self.open - ar[1:] + self.ext)
            H[i] = h
            hp, fp = np.concatenate(([0], h)), f
        return H

    def summary(self, q3, qa, t3, ta):
        """(score, qend, tend) with the oracle's tie-break, and the rows that hold an optimal cell"""
        H = self.H(q3, qa, t3, ta)
        b = int(H.max())
        if b == 0:
            return (0, -1, -1), np.zeros(0, int)
        j = int(np.nonzero(H.max(0) == b)[0][0])
        i = int(np.nonzero(H[:, j] == b)[0][0])
        return (b, i, j), np.nonzero(H.max(1) == b)[0]
