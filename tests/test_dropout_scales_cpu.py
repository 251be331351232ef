"""Host-side pieces of attention dropout, without a GPU: the backward's scales (ops.backward_scales, the grad_scale
contract of include/bevrender_hip.h with D Pmax in place of Pmax) and the row selection of the host keep mask."""
import math

import numpy as np
import torch

from bevrender_amd import ops


def _draws(n, seed):
    r = np.random.RandomState(seed)
    bound = 2.0 ** r.uniform(-30, 30, n)
    pmax_log2 = np.minimum(r.uniform(-62, 2, n), 0.0)            # as the backward clamps it: [-60, 0]
    pmax_log2 = np.maximum(pmax_log2, -60.0)
    thr = r.choice([0, 1, 2, 17, 6554, 19661, 32768, 49152, 58982, 63570, 64881, 65535], n)
    return bound, pmax_log2, thr


def test_backward_scales_keep_every_bound_with_dropout():
    for f16 in (False, True):
        for bound, pl, thr in zip(*_draws(400, 3 + f16)):
            gs = ops.backward_scales(torch.tensor(bound, dtype=torch.float64), torch.tensor(pl, dtype=torch.float64),
                                     f16, int(thr)).double()
            Dd = 65536.0 / (65536.0 - thr)
            pmax = 2.0 ** pl
            s, s_inv, kp, c2, inv_kc, inv_k = (gs[i].item() for i in range(6))
            tag = f"f16={f16} bound={bound:.3e} log2 Pmax={pl:.3f} thr={thr}"
            # s D Pmax bound <= 2^30: a fixed-point contribution of bwd_q stays under 2^31 after its rounding
            assert s * Dd * pmax * bound <= 2.0 ** 30, tag
            assert s * s_inv == 1.0 and math.log2(s) == round(math.log2(s)), tag
            # the largest such power of two (a smaller one only costs table-gradient resolution), short of the clamp at
            # 2^100 (2^116 in fp16: s = 2^16 2^e16)
            if math.log2(s) < (116 if f16 else 100):
                assert 2 * s * Dd * pmax * bound > 2.0 ** 30, tag
            if not f16:
                assert (kp, c2, inv_kc, inv_k) == (0.0, 1.0, 1.0, 1.0), tag
                continue
            # fp16 operands: D P' = D P 2^kp and P' (D dP - delta) c2 inside 2^14
            assert kp == round(kp) and pmax * 2.0 ** kp * Dd <= 2.0 ** 14, tag
            assert pmax * 2.0 ** kp * c2 * Dd * bound <= 2.0 ** 14, tag
            assert s == 2.0 ** 16 * 2.0 ** kp * c2, tag
            assert inv_kc * 2.0 ** kp * c2 == 1.0 and inv_k * 2.0 ** kp == 1.0, tag


def test_backward_scales_without_dropout_are_unchanged():
    # drop_thr = 0 is the contract without dropout: Pmax itself
    for f16 in (False, True):
        for bound, pl, _ in zip(*_draws(100, 11 + f16)):
            b, p = torch.tensor(bound, dtype=torch.float64), torch.tensor(pl, dtype=torch.float64)
            gs = ops.backward_scales(b, p, f16)
            if f16:
                kp = math.floor(14.0 - pl)
                e16 = min(max(math.floor(14.0 - math.log2(bound) - pl), -100), 100)
                want = [2.0 ** (e16 + 16), 2.0 ** (-e16 - 16), kp, 2.0 ** (e16 - kp), 2.0 ** -e16, 2.0 ** -kp, 0, 0]
            else:
                e = min(max(math.floor(30.0 - math.log2(bound) - pl), -100), 100)
                want = [2.0 ** e, 2.0 ** -e, 0, 1, 1, 1, 0, 0]
            assert gs.dtype == torch.float32 and gs.tolist() == torch.tensor(want, dtype=torch.float32).tolist()


def test_keep_mask_rows_are_the_full_masks_rows():
    S, N, n_ph = 13, 70, 6
    thr = int(round(0.3 * 65536))
    full = ops.dropout_keep_mask(1234, thr, n_ph, S, N)
    rows = torch.tensor([0, 5, 12, 13, 100, S * S - 1, 5])
    part = ops.dropout_keep_mask(1234, thr, n_ph, S, N, rows=rows)
    assert part.shape == (n_ph, len(rows), N)
    assert torch.equal(part, full[:, rows])
    assert torch.equal(ops.dropout_keep_mask(1234, thr, n_ph, S, N, rows=list(range(S * S))), full)
