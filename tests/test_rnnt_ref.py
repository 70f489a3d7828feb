"""CPU: the float64 transducer restatement (rnnt_ref.py) checked against itself - brute force over every alignment, central
finite differences, closed forms - before tests/test_rnnt_gpu.py holds the kernels to it; and the ABI surface of the feature."""
import numpy as np
import pytest

import rnnt_ref as R


@pytest.mark.parametrize("T,U,V,blank", [(1, 0, 3, 0), (1, 2, 4, 0), (2, 1, 3, 1), (3, 2, 4, 3), (4, 3, 4, 0), (4, 0, 2, 1), (3, 3, 4, 2)])
def test_logp_is_the_sum_over_all_alignments(T, U, V, blank):
    rng = np.random.default_rng(100 * T + 10 * U + V)
    logits = rng.normal(size=(1, T, U + 1, V)) * 2.0
    labels = [v for v in range(V) if v != blank]
    y = [labels[int(i)] for i in rng.integers(0, len(labels), size=U)]
    got = R.rnnt_logp(logits, [T], np.asarray([y], dtype=np.int64).reshape(1, U), [U], blank)[0]
    want = R.brute_force_logp(logits[0], T, y, blank)
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)


def test_gradient_equals_central_differences():
    rng = np.random.default_rng(7)
    B, T, U, V, blank = 3, 5, 3, 5, 2
    logits = rng.normal(size=(B, T, U + 1, V)) * 1.5
    hlens, ulens = np.array([5, 3, 4]), np.array([3, 1, 0])
    targets = np.array([[1, 1, 4], [0, 3, 3], [4, 0, 1]])
    g = np.array([1.0, -0.5, 2.0])
    f = lambda x: float((g * R.rnnt_logp(x, hlens, targets, ulens, blank)).sum())
    got = R.rnnt_grad(logits, hlens, targets, ulens, blank, g)
    h = 1e-5
    worst = 0.0
    for idx in np.ndindex(*logits.shape):
        x = logits.copy()
        x[idx] += h
        up = f(x)
        x[idx] -= 2 * h
        fd = (up - f(x)) / (2 * h)
        worst = max(worst, abs(fd - got[idx]) / (1e-6 * abs(fd) + 1e-9))
        assert abs(fd - got[idx]) <= 1e-6 * abs(fd) + 1e-9, (idx, fd, got[idx])
    for b in range(B):                                                       # exactly zero outside the lattice
        assert not got[b, hlens[b]:].any() and not got[b, :, ulens[b] + 1:].any()
    print(f"worst fraction of rtol 1e-6 (+1e-9): {worst:.3f}")


def test_empty_target_is_a_run_of_blanks_and_infeasible_rows():
    rng = np.random.default_rng(3)
    T, V, blank = 6, 5, 1
    logits = rng.normal(size=(3, T, 3, V))
    targets = np.array([[0, 0], [blank, 2], [7, 2]])
    lp = R.rnnt_logp(logits, [4, T, T], targets, [0, 2, 1], blank)
    assert abs(lp[0] - R.log_softmax(logits[0, :4, 0])[:, blank].sum()) <= 1e-12
    assert lp[1] == -np.inf and lp[2] == -np.inf                             # a blank target, a target >= V
    assert R.rnnt_logp(logits, [0, T, T], np.array([[0, 0], [0, 2], [3, 2]]), [0, 2, 1], blank)[0] == -np.inf
    assert not R.rnnt_grad(logits, [4, T, T], targets, [0, 2, 1], blank)[1:].any()


def test_joint_combine_gradients_by_differences():
    rng = np.random.default_rng(11)
    B, T, U1, J = 2, 3, 3, 4
    e, p, dz = rng.normal(size=(B, T, J)), rng.normal(size=(B, U1, J)), rng.normal(size=(B, T, U1, J))
    hlens, ulens = [3, 2], [1, 2]
    f = lambda e_, p_: float((R.joint_combine(e_, p_, hlens, ulens, "tanh") * dz).sum())
    de, dp = R.joint_combine_grad(e, p, dz, hlens, ulens, "tanh")
    h = 1e-6
    for arr, grad, which in ((e, de, 0), (p, dp, 1)):
        for idx in np.ndindex(*arr.shape):
            a, b = arr.copy(), arr.copy()
            a[idx] += h
            b[idx] -= h
            fd = (f(a, p) - f(b, p)) / (2 * h) if which == 0 else (f(e, a) - f(e, b)) / (2 * h)
            assert abs(fd - grad[idx]) <= 1e-7 * max(1.0, abs(fd)), (which, idx, fd, grad[idx])
    z = R.joint_combine(e, p, hlens, ulens, "tanh")
    assert not z[1, 2:].any() and not z[0, :, 2:].any() and z[0, 2, 1].any()


def hand_head():
    """V = 3 (blank 0), joint 3, context 1, no activation: the logits are enc + the embedding of the last token."""
    eye = np.eye(3)
    sd = {"embed.weight": np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 5.0], [6.0, 0.0, 0.0]]),      # after 1: favour 2; after 2: favour blank
          "pred.weight": eye, "pred.bias": np.zeros(3), "enc_proj.weight": eye, "enc_proj.bias": np.zeros(3),
          "pred_proj.weight": eye, "out.weight": eye, "out.bias": np.zeros(3)}
    return R.Head(sd, blank=0, context=1, activation="none")


def test_greedy_reference_on_a_hand_built_case():
    head = hand_head()
    enc = np.array([[[0.0, 4.0, 1.0],        # frame 0: 1, then (after 1: +5 on 2) 2, then (after 2: +6 on blank) blank
                     [3.0, 0.0, 0.0],        # frame 1: blank at once after 2; after 1 it is 2
                     [2.0, 0.0, 0.0],        # frame 2: blank
                     [0.0, 9.5, 0.0]]])      # frame 3 (beyond hlens = 3): 1 whatever came before
    toks, frames, margins = head.greedy(enc, [3], max_symbols_per_frame=3)
    assert toks == [[1, 2]] and frames == [[0, 0]]
    assert len(margins[0]) == 5 and np.allclose(margins[0], [3.0, 2.0, 2.0, 9.0, 8.0], atol=1e-12)
    toks, frames, _ = head.greedy(enc, [3], max_symbols_per_frame=1)        # one symbol per frame: the 2 moves to frame 1
    assert toks == [[1, 2]] and frames == [[0, 1]]
    toks, frames, _ = head.greedy(enc, [4], max_symbols_per_frame=3)        # frame 3 emits until the cap
    assert toks == [[1, 2, 1, 1, 1]] and frames == [[0, 0, 3, 3, 3]]


def test_head_loss_matches_its_parts():
    rng = np.random.default_rng(5)
    V, D, J, B, T, U = 6, 4, 5, 2, 4, 2
    sd = {"embed.weight": rng.normal(size=(V, J)), "pred.weight": rng.normal(size=(J, 2 * J)), "pred.bias": rng.normal(size=J),
          "enc_proj.weight": rng.normal(size=(J, D)), "enc_proj.bias": rng.normal(size=J), "pred_proj.weight": rng.normal(size=(J, J)),
          "out.weight": rng.normal(size=(V, J)), "out.bias": rng.normal(size=V)}
    head = R.Head(sd)
    ys = np.array([[3, 1], [2, 5]])
    ctx = head.contexts(ys, U + 1)
    assert ctx.tolist() == [[[0, 0], [0, 3], [3, 1]], [[0, 0], [0, 2], [2, 5]]]
    enc = rng.normal(size=(B, T, D))
    loss, lp = head.loss(enc, [4, 3], ys, [2, 1])
    assert np.isfinite(lp).all() and abs(loss + lp.sum() / B) <= 1e-12
    # the written-out chain rule against central differences of the loss, a few entries of every weight and of enc
    loss2, grads, denc, _ = head.loss_and_grads(enc, [4, 3], ys, [2, 1])
    assert abs(loss2 - loss) <= 1e-12 and sorted(grads) == sorted(sd)

    def diff(arr, idx):
        keep = arr[idx]
        arr[idx] = keep + 1e-6
        up = head.loss(enc, [4, 3], ys, [2, 1])[0]
        arr[idx] = keep - 1e-6
        down = head.loss(enc, [4, 3], ys, [2, 1])[0]
        arr[idx] = keep
        return (up - down) / 2e-6

    for name, gr in list(grads.items()) + [("enc", denc)]:
        arr = enc if name == "enc" else head.w[name]
        for _ in range(6):
            idx = tuple(int(rng.integers(0, n)) for n in arr.shape)
            if name == "embed.weight":
                idx = (int(rng.choice([0, 3, 2])),) + idx[1:]                # rows the contexts use
            fd = diff(arr, idx)
            assert abs(fd - gr[idx]) <= 1e-6 * max(1.0, abs(fd)), (name, idx, fd, gr[idx])
    assert not denc[1, 3:].any() and not grads["embed.weight"][4].any()


def test_the_library_carries_the_transducer_abi():
    """The exports, the limits and the size function of the new entries (no launch: CPU)."""
    from openeat_amd import hip
    lib = hip.lib()
    assert lib.oe_abi_version() >= 10
    up16 = lambda n: (n + 15) // 16 * 16
    for B, T, U in ((8, 250, 30), (1, 1, 0), (3, 8192, 255), (2, 7, 63)):
        N = B * T * (U + 1)
        assert lib.oe_rnnt_workspace_bytes(B, T, U) == 3 * up16(4 * N) + 2 * up16(8 * N) + up16(8 * B) + up16(4 * B)
    for B, T, U in ((0, 5, 3), (1, 0, 3), (1, 8193, 3), (1, 5, -1), (1, 5, 256), (1200, 8192, 255)):
        assert lib.oe_rnnt_workspace_bytes(B, T, U) == 0
    a = hip.RnntArgs()
    assert lib.oe_rnnt_loss(hip.C.byref(a), None) != 0 and b"null" in lib.oe_last_error()
    assert lib.oe_rnnt_grad(None, None) != 0 and b"null" in lib.oe_last_error()
    assert lib.oe_joint_combine_fwd(hip.C.byref(hip.JointCombineArgs()), None) != 0 and b"null" in lib.oe_last_error()
    assert lib.oe_joint_combine_bwd(hip.C.byref(hip.JointCombineBwdArgs()), None) != 0 and b"null" in lib.oe_last_error()
