"""Shared by the grand-product tests (CPU and GPU): the layered product argument of a column A of n = 2^v canonical words restated
in Python ints / numpy on oracle_lib.Transcript.

    V_v = A,  V_j[x] = V_{j+1}[x] * V_{j+1}[x + 2^j] (x < 2^j),  L_j = V_{j+1}[:2^j],  H_j = V_{j+1}[2^j:],  product = V_0[0].

ONE transcript per instance: it absorbs the product; layer 0 writes l_0 = V_1[0], h_0 = V_1[1], absorbs them and draws c_0; layer
j >= 1 is the closed-form zero-check of sum_x eq(tau^(j), x) L_j(x) H_j(x) -- zerocheck_closed_ref.prove over (L_j, H_j), term
(1, (0, 1)), at the layer's challenges, j rounds of 4 coefficients, each absorbed and drawn from in turn --, then l_j = L_j(q),
h_j = H_j(q) at q = the round challenges reversed are absorbed and c_j drawn; tau^(j+1) = (q, c_j), claim_(j+1) = l_j + c_j (h_j -
l_j).  Points are in Multilinear.eval's convention (coordinate 0 with the LSB of the index).  With fixed challenges (v (v + 1) / 2
words in order of use: c_0, layer 1's round challenge, c_1, layer 2's two, c_2, ...) there is no transcript.

A proof is (product, layer_evals [2 v], rounds [2 v (v - 1)], points [v (v - 1) / 2], layer_challenges [v], leaf_point [v],
leaf_eval).  Everything is exact."""
import numpy as np

import exact_ref
import oracle_lib as O
import sop_ref as S
import zerocheck_closed_ref as ZC
import zerocheck_ref as Z

P = O.P_BB
_P = np.uint64(P)
TERM = [(1, (0, 1))]


def layers(col):
    """[V_0, V_1, .., V_v] (np.uint64 arrays)"""
    out = [np.ascontiguousarray(col, dtype=np.uint64)]
    while len(out[0]) > 1:
        h = len(out[0]) // 2
        out.insert(0, (out[0][:h] * out[0][h:]) % _P)
    return out


def tree_buffer(col, fill=0):
    """the n words of the layers entry's output: layer j at word n - 2^(j+1); word n - 1 holds `fill`"""
    V = layers(col)
    n = len(col)
    buf = np.full(n, fill, dtype=np.uint64)
    for j in range(len(V) - 1):
        buf[n - (2 << j): n - (2 << j) + (1 << j)] = V[j]
    return buf


def fixed_words(v):
    return v * (v + 1) // 2


def _layer(L, H, tau, claim, tr, fixed):
    """layer j >= 1: (rounds, round challenges, l, h).  Fiat-Shamir: the rounds are formed one by one against the shared transcript
    (the sum-of-products reference's round over the pool (L, H, eq), which is what zerocheck_closed_ref.prove runs), and the
    layer's proof is then zerocheck_closed_ref.prove at the challenges drawn -- the two must agree word for word"""
    j = len(tau)
    if fixed is None:
        pool, terms = ZC.table_route([L, H], TERM, Z.eq_table(tau))
        fs = [np.ascontiguousarray(t, dtype=np.uint64).copy() for t in pool]
        drawn, seen = [], []
        for _ in range(j):
            c = S.round_coefficients(fs, terms)
            seen += c
            for x in c:
                tr.append_field(x)
            ch = tr.challenge()
            drawn.append(ch)
            half = len(fs[0]) // 2
            fs = [(f[:half] + (np.uint64(ch) * ((f[half:] + _P - f[:half]) % _P)) % _P) % _P for f in fs]
        fixed = drawn
    else:
        seen = None
    claimed, rounds, point, evals, eq_eval, fe = ZC.prove([L, H], TERM, tau, [int(x) for x in fixed])
    assert seen is None or [int(x) for x in rounds] == seen
    assert int(claimed) == claim, "the honest chain closes at every layer"
    q = [int(x) for x in point][::-1]
    assert int(eq_eval) == Z.eq_at(tau, q) and int(fe) == int(eq_eval) * int(evals[0]) % P * int(evals[1]) % P
    return [int(x) for x in rounds], [int(x) for x in point], int(evals[0]), int(evals[1])


def prove(col, challenges=None):
    V = layers(col)
    v = len(V) - 1
    assert v >= 1
    fixed = None if challenges is None else [int(x) for x in challenges]
    assert fixed is None or len(fixed) == fixed_words(v)
    tr = O.Transcript()
    product = int(V[0][0])
    if fixed is None:
        tr.append_field(product)
    evals, rounds, points, chs = [], [], [], []
    tau, claim = [], product
    for j in range(v):
        L, H = V[j + 1][:1 << j], V[j + 1][1 << j:]
        if j == 0:
            l, h, q = int(L[0]), int(H[0]), []
        else:
            r, pts, l, h = _layer(L, H, tau, claim, tr, None if fixed is None else fixed[j * (j + 1) // 2: j * (j + 1) // 2 + j])
            rounds += r
            points += pts
            q = pts[::-1]
        evals += [l, h]
        if fixed is None:
            tr.append_field(l)
            tr.append_field(h)
            c = tr.challenge()
        else:
            c = fixed[j * (j + 1) // 2 + j]
        chs.append(c)
        tau = q + [c]
        claim = (l + c * (h - l)) % P
    u = lambda a: np.array(a, dtype=np.uint64)  # noqa: E731
    return product, u(evals), u(rounds), u(points), u(chs), u(tau), claim


def same(a, b):
    return (int(a[0]) == int(b[0]) and int(a[6]) == int(b[6])
            and all(np.array_equal(np.asarray(a[i], dtype=np.uint64), np.asarray(b[i], dtype=np.uint64)) for i in range(1, 6)))


def _horner(c, x):
    s = 0
    for y in reversed(c):
        s = (s * x + int(y)) % P
    return s


def replay(proof):
    """(layers_ok, expected, leaf_point): every challenge derived from the one transcript; expected is the claim at the failing
    step (the product check, a round's g(0) + g(1), a layer's eq * l * h) or claim_v"""
    product, evals, rounds = int(proof[0]), [int(x) for x in proof[1]], [int(x) for x in proof[2]]
    v = len(evals) // 2
    tr = O.Transcript()
    tr.append_field(product)
    claim, tau, ro = product, [], 0
    for j in range(v):
        l, h = evals[2 * j], evals[2 * j + 1]
        q = [0] * j
        for x in range(j):
            c = rounds[ro: ro + 4]
            ro += 4
            if (2 * c[0] + c[1] + c[2] + c[3]) % P != claim:
                return False, claim, None
            for y in c:
                tr.append_field(y)
            ch = tr.challenge()
            claim = _horner(c, ch)
            q[j - 1 - x] = ch
        if Z.eq_at(tau, q) * l % P * h % P != claim:
            return False, claim, None
        tr.append_field(l)
        tr.append_field(h)
        c = tr.challenge()
        tau = q + [c]
        claim = (l + c * (h - l)) % P
    return True, claim, tau


def verdict(col, proof, leaf_deferred=False, mle_eval=exact_ref.eval):
    """(accept, expected_eval, oracle_eval): accept iff the layers hold, the derived leaf point is the proof's, leaf_eval is
    claim_v and -- unless the leaf is deferred to the caller (oracle_eval is then None) -- so is the column's evaluation at the
    proof's leaf point"""
    ok, expected, leaf = replay(proof)
    given = [int(x) for x in proof[5]]
    oracle = None if leaf_deferred else int(mle_eval(np.ascontiguousarray(col, dtype=np.uint64), given))
    good = ok and leaf == given and int(proof[6]) == expected and (leaf_deferred or oracle == expected)
    return bool(good), int(expected), oracle


TAMPERS = ("product", "layer_eval_0", "layer_eval_mid", "round", "leaf_point", "leaf_eval", "column")


def tampered(col, proof):
    """{name: (column, proof)} for every name of TAMPERS: the honest instance with ONE thing changed.  A word changes by + 1 mod p;
    "column" changes one leaf."""
    product, evals, rounds, points, chs, leaf, le = proof
    evals, rounds, leaf = (np.asarray(a, dtype=np.uint64) for a in (evals, rounds, leaf))
    v = len(leaf)

    def bump(a, i):
        b = a.copy()
        b[i] = (int(b[i]) + 1) % P
        return b

    out = {
        "product": (col, ((int(product) + 1) % P, evals, rounds, points, chs, leaf, le)),
        "layer_eval_0": (col, (product, bump(evals, 0), rounds, points, chs, leaf, le)),
        "layer_eval_mid": (col, (product, bump(evals, 2 * (v // 2) + 1), rounds, points, chs, leaf, le)),
        "round": (col, (product, evals, bump(rounds, len(rounds) // 2 + 1), points, chs, leaf, le)),
        "leaf_point": (col, (product, evals, rounds, points, chs, bump(leaf, v // 2), le)),
        "leaf_eval": (col, (product, evals, rounds, points, chs, leaf, (int(le) + 1) % P)),
        "column": (bump(np.asarray(col, dtype=np.uint64), len(col) // 3), proof),
    }
    assert tuple(out) == TAMPERS
    return out


COLUMN_KINDS = ("random", "all_pm1", "all_one", "one_zero", "one_not_one")


def column(kind, v, seed=0):
    """the five column kinds of the tests at 2^v: random; all p - 1; all 1; one zero leaf (every layer above it is zero on a path);
    a single leaf that is not one"""
    n = 1 << v
    if kind == "random":
        return O.splitmix64_field(9900 + seed + 31 * v, n)
    if kind == "all_pm1":
        return np.full(n, P - 1, dtype=np.uint64)
    a = np.ones(n, dtype=np.uint64) if kind != "one_zero" else O.splitmix64_field(9950 + seed + 31 * v, n)
    if kind == "one_zero":
        a[(5 * n) // 7] = 0
    elif kind == "one_not_one":
        a[(2 * n) // 3] = 123456789
    else:
        assert kind == "all_one"
    return a


EDGE_WORDS = (0, 1, (P + 1) // 2, P - 1)


def edge_challenges(v, seed=0):
    """v (v + 1) / 2 fixed challenges drawn from 0, 1, (p + 1) / 2, p - 1 and random words, a different place for every seed"""
    c = [int(x) for x in O.splitmix64_field(9970 + seed, fixed_words(v))]
    for i in range(len(c)):
        if (i + seed) % 2 == 0:
            c[i] = EDGE_WORDS[(i // 2 + seed) % 4]
    return c


_PINNED = {}


def pinned(v):
    """(column, proof) for the tamper tests at 2^v, computed once: the first seed at which the reference rejects EVERY tamper,
    chosen as zerocheck_closed_ref.pinned chooses its seed, so that no tamper is ever dropped"""
    if v not in _PINNED:
        for seed in range(9600 + 100 * v, 9600 + 100 * v + 30, 10):
            col = O.splitmix64_field(seed, 1 << v)
            proof = prove(col)
            assert verdict(col, proof)[0]
            if all(not verdict(*t)[0] for t in tampered(col, proof).values()):
                _PINNED[v] = (col, proof)
                break
        else:
            raise AssertionError("no seed at which the reference rejects every tamper")
    return _PINNED[v]
