"""The exchange ring of the cooperative grid (csrc/kernels_coop.inc, "pair units"), as a model on the CPU.

Values travel untagged; "not yet written" is a sentinel, and an owner resets its own slot of the buffer two rounds
on.  The model has what the argument in the source rests on and nothing else:

* a workgroup publishes round k (value into buffer k % B, sentinel into its slot of buffer (k + reset) % B), gathers
  round k (polls every slot of buffer k % B in any order until it differs from the sentinel), and only then goes on;
* a store becomes visible at ANY time between its issue and the acknowledgement, which is the end of the same
  workgroup's gather of that round (s_waitcnt vmcnt(0)); two stores in flight may land in either order, except that
  stores of one lane to one address keep their order.

A reader must never accept a value of another round, and the grid must not hang.  Four buffers with a reset two rounds
on hold under every schedule tried; three buffers do not, whichever buffer the reset goes to.
"""
import os
import random
import re

import pytest

SENT = None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def simulate(groups, rounds, nbuf, reset, seed, max_steps=200000):
    """-> None, or a string that says what went wrong"""
    rng = random.Random(seed)
    buf = [[SENT] * groups for _ in range(nbuf)]
    rnd = [1] * groups  # the round a workgroup is in
    todo = [None] * groups  # slots it still misses in its gather (None: it has not published yet)
    flight = [[] for _ in range(groups)]  # its stores not yet visible: (buffer, value), in issue order
    for _ in range(max_steps):
        live = [g for g in range(groups) if rnd[g] <= rounds]
        if not live:
            return None
        acts = [("step", g) for g in live] + [("land", g) for g in range(groups) if flight[g]]
        kind, g = rng.choice(acts)
        if kind == "land":
            # any store in flight may land, but not before an earlier one of this workgroup to the same buffer (same address)
            cands = [i for i, (b, _) in enumerate(flight[g]) if all(flight[g][j][0] != b for j in range(i))]
            b, v = flight[g].pop(rng.choice(cands))
            buf[b][g] = v
            continue
        k = rnd[g]
        if todo[g] is None:
            flight[g].append((k % nbuf, (g, k)))
            flight[g].append(((k + reset) % nbuf, SENT))
            todo[g] = set(range(groups))
            continue
        if todo[g]:
            s = rng.choice(sorted(todo[g]))
            v = buf[k % nbuf][s]
            if v is not SENT:
                if v != (s, k):
                    return "workgroup %d in round %d accepted slot %d of round %d" % (g, k, s, v[1])
                todo[g].discard(s)
            continue
        for b, v in flight[g]:  # the gather is over: everything this workgroup stored is acknowledged
            buf[b][g] = v
        flight[g] = []
        todo[g] = None
        rnd[g] += 1
    return "no progress: workgroups in rounds %s" % rnd


@pytest.mark.parametrize("groups", [2, 3, 5])
def test_four_buffers_never_hand_over_another_rounds_value(groups):
    for seed in range(60):
        assert simulate(groups, 9, 4, 2, seed) is None, seed


def test_three_buffers_are_not_enough():
    # reset one round on, (k + 1) % 3: a reader that has seen this owner's round k enters round k + 1 before the reset
    # has landed and accepts what round k - 2 left there
    stale = [simulate(3, 10, 3, 1, seed) for seed in range(80)]
    assert any(s and "accepted" in s for s in stale)
    # reset two rounds on, (k + 2) % 3 = (k - 1) % 3: it hits the buffer slower workgroups still gather
    racy = [simulate(3, 10, 3, 2, seed) for seed in range(80)]
    assert any(racy)
    # (and four buffers with a reset ONE round on are as bad as three: the distance of two is what the argument needs)
    assert any(simulate(3, 10, 4, 1, seed) for seed in range(80))


def ring_slot(c, B=512):
    """8-byte word of column c in a buffer: coop_ring_slot<B>"""
    return 2 * ((c // (2 * B)) * B + c % B) + ((c // B) & 1)


def pick_cpt(NR):
    return 2 if NR < 1024 else 3 if NR < 1536 else 4


def test_the_model_of_the_slot_map_is_the_sources():
    src = open(os.path.join(ROOT, "miosqp_amd", "csrc", "kernels_coop.inc")).read()
    host = open(os.path.join(ROOT, "miosqp_amd", "csrc", "host.inc")).read()
    assert "return 2 * (size_t)((c / (2 * COOP_B)) * COOP_B + c % COOP_B) + (size_t)((c / COOP_B) & 1);" in src
    assert "int coop_pick_cpt(int NR) { return NR < 1024 ? 2 : NR < 1536 ? 3 : 4; }" in host
    m = re.search(r"COOP_RING_WORDS = (\d+);", src)
    assert m and int(m.group(1)) > ring_slot(2048)
    m = re.search(r"COOP_SENTINEL = 0x([0-9A-Fa-f]+)ull", src)
    bits = int(m.group(1), 16)
    # a signalling NaN: exponent all ones, quiet bit clear, payload non-zero
    assert (bits >> 52) & 0x7FF == 0x7FF and not (bits >> 51) & 1 and bits & ((1 << 51) - 1)


def test_slot_map_is_a_bijection_onto_distinct_slots():
    for NR in range(193, 2049):
        cpt = pick_cpt(NR)
        slots = [ring_slot(c) for c in range(NR + 1)]  # the testers' decision, column NR, included
        assert len(set(slots)) == NR + 1, NR
        assert max(slots) < 4096
        # thread t finds its columns k = 2 u, 2 u + 1 in the two halves of unit u * 512 + t
        for t in (0, 1, 255, 511):
            for k in range(cpt):
                c = t + k * 512
                if c <= NR:
                    assert ring_slot(c) == 2 * ((k // 2) * 512 + t) + (k & 1)
