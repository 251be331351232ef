"""The host side of the tap route for two channel groups, in plain torch and float64 (no GPU): the per-(problem, group)
key orders of ops.tap_group_order, and the algebra of the route -- per-group pixel rows (ops.tap_group_pixels), logits
as a sum over both groups' tap weights, the bias of a head from its own group's positions, O = sum_g' Rn^g' Vpix^g' + bv
-- against the oracle's SCA forward with n_groups = 2 (reference model/SCA_deform_attn.py:290-413) when every key is
pinned."""
import os
import sys

import torch
import torch.nn.functional as F

from bevrender_amd import ops
from oracle import bevrender_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def _rows(P=3, N=97, seed=0):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(P * 2, N, generator=gen, dtype=torch.float64) * 9
    b = torch.rand(P * 2, N, generator=gen, dtype=torch.float64) * 30
    ys = torch.rand(P * 2, N, generator=gen, dtype=torch.float64) * 3 - 1
    xs = torch.rand(P * 2, N, generator=gen, dtype=torch.float64) * 2 - 1
    return a, b, ys, xs


def test_every_row_has_a_permutation_of_its_own_and_is_cell_sorted():
    a, b, ys, xs = _rows()
    order, a_o, b_o, y_o, x_o = ops.tap_group_order(a, b, ys, xs, 2)
    R, N = a.shape
    assert order.shape == (R, N) and y_o.shape == x_o.shape == (R, 2, N)
    assert torch.equal(order.sort(1).values, torch.arange(N).expand(R, N))
    assert torch.equal(order, ops.cell_order(a, b))               # each row by its OWN group's table coordinates
    assert not torch.equal(order[0], order[1])                    # the two groups of a problem are ordered independently
    assert torch.equal(a_o, a.gather(1, order)) and torch.equal(b_o, b.gather(1, order))
    cell = torch.floor(a_o)
    assert (cell[:, 1:] >= cell[:, :-1]).all()                    # table rows ascending: cell-sorted


def test_a_row_holds_both_groups_positions_of_the_same_keys():
    a, b, ys, xs = _rows(seed=1)
    order, _, _, y_o, x_o = ops.tap_group_order(a, b, ys, xs, 2)
    for r in range(a.shape[0]):
        p = r // 2
        for g2 in range(2):
            assert torch.equal(y_o[r, g2], ys[p * 2 + g2][order[r]]), (r, g2)
            assert torch.equal(x_o[r, g2], xs[p * 2 + g2][order[r]]), (r, g2)


def test_gradients_come_back_through_the_gathers_to_the_right_group_and_key():
    a, b, ys, xs = _rows(P=2, N=40, seed=2)
    leaves = [t.clone().requires_grad_(True) for t in (a, b, ys, xs)]
    order, a_o, b_o, y_o, x_o = ops.tap_group_order(*leaves, 2)
    R, N = a.shape
    gen = torch.Generator().manual_seed(3)
    ca, cb = (torch.randn(R, N, generator=gen, dtype=torch.float64) for _ in range(2))
    cy, cx = (torch.randn(R, 2, N, generator=gen, dtype=torch.float64) for _ in range(2))
    ((a_o * ca).sum() + (b_o * cb).sum() + (y_o * cy).sum() + (x_o * cx).sum()).backward()
    inv = order.argsort(1)                                        # key n sits at index inv[r][n] of row r
    assert torch.equal(leaves[0].grad, ca.gather(1, inv)) and torch.equal(leaves[1].grad, cb.gather(1, inv))
    for p in range(R // 2):
        for g2 in range(2):
            # group g2's position of key n is used by BOTH rows of its problem, each at its own index
            want_y = sum(cy[p * 2 + g, g2][inv[p * 2 + g]] for g in range(2))
            want_x = sum(cx[p * 2 + g, g2][inv[p * 2 + g]] for g in range(2))
            assert torch.allclose(leaves[2].grad[p * 2 + g2], want_y, rtol=0, atol=1e-14)
            assert torch.allclose(leaves[3].grad[p * 2 + g2], want_x, rtol=0, atol=1e-14)
    # a single cotangent entry lands on one (group, key)
    leaves = [t.clone().requires_grad_(True) for t in (a, b, ys, xs)]
    order, _, _, y_o, _ = ops.tap_group_order(*leaves, 2)
    y_o[3, 0, 7].backward()               # row 3 = (problem 1, group 1), plane 0, index 7
    g = leaves[2].grad
    assert g.abs().sum() == 1.0 and g[2, order[3, 7]] == 1.0


def test_group_pixel_rows_sum_to_the_one_group_rows():
    gen = torch.Generator().manual_seed(4)
    feat = torch.randn(3, 3, 5, 8, generator=gen, dtype=torch.float64)       # 3 rows only: the fourth is zero padding
    W = torch.randn(16, 8, generator=gen, dtype=torch.float64)
    kvp = ops.tap_group_pixels(feat, W, 2)
    assert kvp.shape == (3, 24, 16) and kvp.dtype == torch.float64
    one = F.linear(F.pad(feat[:, :4, :3], (0, 0, 0, 0, 0, 1)).reshape(3, 12, 8), W)
    assert torch.allclose(kvp[:, :12] + kvp[:, 12:], one, rtol=0, atol=1e-13)
    assert torch.allclose(kvp[:, 12:], F.linear(F.pad(feat[:, :4, :3, 4:], (0, 0, 0, 0, 0, 1)).reshape(3, 12, 4), W[:, 4:]),
                          rtol=0, atol=1e-13)
    assert kvp[:, 9:12].abs().max() == 0 and kvp[:, 21:24].abs().max() == 0


def test_the_grouped_tap_algebra_reproduces_the_oracle_when_every_key_is_pinned():
    """S = 8: 4 x 16 keys per view, all with their reference at (-1, -1); offsets inside the tap grid (Hi = 4, and
    2.5 (Wi - 1) / (Wk - 1) = 1.5 < 2).  Every (problem, group) row in its own cell order."""
    import tap_check as tc
    from bevrender_amd.model.SCA_deform_attn import SCADeformableAttention
    B, V, C, h, g, S, D, Hi, Wi = 2, 2, 16, 4, 2, 8, 2, 4, 10
    torch.manual_seed(11)
    m = SCADeformableAttention(bev_feat_shape=S, bev_depth_dim=D, dim_embed=C, n_heads=h, n_groups=g, stride=1,
                               kernel_size=3, scale_offset_range=True, batch_size=B, n_views=V)
    gen = torch.Generator().manual_seed(12)
    p = {n: (torch.randn(v.shape, generator=gen) * 0.4).double() for n, v in m.state_dict().items()}
    query = torch.randn(B, C, S, S, generator=gen).double()
    x = torch.randn(B, V, C, Hi, Wi, generator=gen).double()
    Hk, Wk = S // 2, S * D
    N, M, c = Hk * Wk, S * S, C // h
    ref = torch.full((B, V, Hk, Wk, 2), -1.0, dtype=torch.float64)
    want = O.sca_forward(p, x, query, ref, n_heads=h, n_groups=g, depth_dim=D, scale_offset_range=True)

    Wkv = torch.cat((p["proj_k.weight"].flatten(1), p["proj_v.weight"].flatten(1)), 0)
    bkv = torch.cat((p["proj_k.bias"], p["proj_v.bias"]), 0)
    table = p["rpe_table"]
    Wt = table.shape[-1]
    q_grid = O.normalized_grid(S, S, torch.float64).reshape(M, 2)
    outs = []
    for v in range(V):
        pos = O.sca_key_positions(p, query, ref[:, v].repeat_interleave(g, dim=0)[..., (1, 0)], v, g, D, True).reshape(B * g, N, 2)
        ys, xs = (pos[..., 0] + 1) * 0.5 * (Hi - 1), (pos[..., 1] + 1) * 0.5 * (Wi - 1)
        assert ys.max() < ops.TAP_R - 1 and xs.max() < ops.TAP_C - 1
        a, b = ops.key_coords(pos, S, Wt, N)
        order, _, _, y_o, x_o = ops.tap_group_order(a.double(), b.double(), ys, xs, g)
        kvp = ops.tap_group_pixels(x[:, v].permute(0, 2, 3, 1), Wkv, g)                    # (B, 24, 2C)
        o_v = torch.zeros(B, C, M, dtype=torch.float64)
        for bi in range(B):
            for hd in range(h):
                r = bi * g + hd // (h // g)                       # the head's record row
                ch = slice(hd * c, (hd + 1) * c)
                Q = query[bi, ch].reshape(c, M).t() * c ** -0.5                             # (M, c)
                w = torch.cat([tc.tap_w(y_o[r, g2], x_o[r, g2])[:, :12] for g2 in range(g)], 1)    # (N, 24) in row r's order
                G = Q @ kvp[bi, :, :C][:, ch].t()                                           # (M, 24)
                Gb = Q @ bkv[:C][ch]
                pr = pos[r][order[r]]                             # the head's own group's positions, in that order
                disp = (q_grid[:, None] - pr[None]) * 0.5
                bias = F.grid_sample(table[hd][None, None], disp[None][..., (1, 0)], mode="bilinear", align_corners=True)[0, 0]
                Pm = torch.softmax(G @ w.t() + Gb[:, None] + bias, dim=1)                   # (M, N)
                Rn = Pm @ w                                                                 # (M, 24)
                o_v[bi, ch] = (Rn @ kvp[bi, :, C:][:, ch] + bkv[C:][ch]).t()
        outs.append(o_v.reshape(B, C, S, S))
    got = F.conv2d(torch.cat(outs, 1), p["proj_out.weight"], p["proj_out.bias"])
    assert (got - want).abs().max().item() < 1e-10 * max(1.0, want.abs().max().item())
