"""The C oracle's hit ORDER, pinned against an expectation that does not use
its walker.

Every GPU test takes the order of a topic's values from Oracle.matches /
match_batch; test_oracle_golden.py::test_walker_equals_spec_matcher compares
sorted sets, so only the golden vectors pinned that order.  Here: the keys the
brute-force spec matcher accepts, sorted in Erlang term order of the key
(emqx_amd.trie_search.key_order: word lists before binaries, words in byte
order, '#' < '+' < any binary word) and then by value, must equal
Oracle.matches(t) as a list -- over the full byte range (bytes_vocab), binary
and word-list keys, several values per filter and full-range u32 values.

Stored filters carry '#' as their last level only: the reference's walk skips
keys after a non-final '#' (test_oracle_golden.py::test_reference_quirk_hash_not_last).
"""
import random

import pytest

from bytes_vocab import full_range_values, short_vocabulary
from emqx_amd.trie_search import BadArg, filter_words, key_order, make_key, topic_words
from pyoracle import Oracle, spec_match

VOCAB = short_vocabulary()


def _filter(r, pool):
    n = r.randint(1, 5)
    ws = [b"+" if r.random() < 0.25 else r.choice(pool) for _ in range(n)]
    if r.random() < 0.25:
        ws = ws[:r.randint(0, n - 1)] + [b"#"]          # '#' last only
    return b"/".join(ws)


@pytest.mark.parametrize("seed", range(40))
def test_walker_order_is_key_order_then_value(seed):
    r = random.Random(0x0DE7 * 1000 + seed)
    # a small pool per seed, so that filters share prefixes and topics hit several keys;
    # the NUL runs, the '$' words and the high-bit twins are in every pool
    pool = r.sample(VOCAB, 10) + [b"", b"\0", b"\0\0", b"$", b"\xa4", b"\xaf", b"\xab", b"\xa3", b"a", b"a\0"]
    filters = [_filter(r, pool) for _ in range(90)]
    vals = full_range_values(r, 12)
    o = Oracle()
    keys = {}                                             # key -> (filter bytes, words form)
    for f in filters:
        for _ in range(r.choice([1, 1, 2, 4])):           # several values on one filter
            v = r.choice(vals)
            wf = r.random() < 0.3                         # a word-list key (flags 1)
            o.insert(f, v, 1 if wf else 0)
            keys[make_key(tuple(filter_words(f)) if wf else f, v)] = (f, wf)
    assert o.size() == len(keys)
    for k, (f, _) in keys.items():
        ws = k[0] if isinstance(k[0], tuple) else ()
        assert "#" not in ws[:-1], f
    topics = []
    for f in filters:
        ws = [r.choice(pool) if w in (b"+", b"#") else w for w in f.split(b"/")]
        if r.random() < 0.3:
            ws += [r.choice(pool) for _ in range(r.randint(1, 2))]
        if r.random() < 0.2:
            ws[r.randrange(len(ws))] = r.choice(pool)
        topics.append(b"/".join(ws))
    topics += [b"", b"/", b"//", b"$", b"$/\0", b"\xa4", b"\xa4/\0", b"\0", b"\0\0/\0", b"+", b"a/#", b"\0/+/a", b"#/\0"]
    n_bad = n_hit = n_multi = 0
    for t in topics:
        got = o.matches(t)
        try:
            topic_words(t)
        except BadArg:
            assert got is None, t
            n_bad += 1
            continue
        acc = [k for k, (f, wf) in keys.items() if spec_match(t, f, wf)]
        acc.sort(key=lambda k: (key_order(k)[0], k[1][0]))
        assert got == [k[1][0] for k in acc], (t, got, acc)
        n_hit += bool(acc)
        n_multi += len(acc) > 2
    assert n_bad >= 4 and n_hit > len(topics) // 2 and n_multi > 5
