"""A word vocabulary over the full byte range, shared by the byte-range tests
(test_gpu_walk_bytes.py, test_oracle_order_cpu.py, test_matches_filter_cpu.py).

MQTT topics are UTF-8 and the reference treats them as arbitrary binaries, so
every byte but '/' may occur inside a level.  The words here are the ones a
tokeniser or a word table can get wrong without an ASCII test noticing:

* every one-byte word 0x00-0xFF except '/', '+' and '#';
* runs of NUL bytes of length 0-9 (the device identifies a short word by its
  first two dwords plus a length: these differ in the length alone), and
  'a', 'a\\0', '\\0a', 'a\\0\\0';
* the high-bit twins of '/', '+', '#' and '$' (0xAF, 0xAB, 0xA3, 0xA4) and the
  neighbours of '/' (0x2E, 0x30), alone and inside words: a word-at-a-time
  zero-byte test that loses bit 7, or is off by one, splits or merges there;
* UTF-8 words of 7, 8, 9, 16 and 17 bytes made of 2-, 3- and 4-byte sequences;
* long words with the same first 8 bytes and the same length that differ in
  their last byte only, or by 0x00 against 0x80;
* words of 251-257 bytes sharing their first 251 / 254 bytes (a length kept in
  one byte saturates at 255; "lit/" + 251..253 bytes is a topic of 255..257
  bytes).
"""

SPECIAL = (0x2F, 0x2B, 0x23)          # '/', '+', '#': never a one-byte word
TWINS = (0xAF, 0xAB, 0xA3, 0xA4)      # '/', '+', '#', '$' with bit 7 set
NEIGHBOURS = (0x2E, 0x30)             # '/' - 1, '/' + 1

_LONG = bytes((37 * i + 11) % 251 + 1 for i in range(257)).replace(b"/", b"\x01")


def one_byte_words():
    return [bytes([b]) for b in range(256) if b not in SPECIAL]


def nul_words():
    return [b"\0" * k for k in range(10)] + [b"a", b"a\0", b"\0a", b"a\0\0"]


def twin_words():
    out = []
    for b in TWINS + NEIGHBOURS:
        c = bytes([b])
        out += [c, c + c, b"x" + c, c + b"x", b"ab" + c + b"cd", b"abcdefg" + c, b"abcdefgh" + c + b"ijklmnop"]
    out += [b"\xa4SYS", b"\xab\xa3", b"a+", b"#a", b"\xaf+", b"+\xaf", b"$\xa4"]
    return out


def utf8_words():
    e, eu, clef = "é".encode(), "€".encode(), "\U0001d11e".encode()   # 2, 3 and 4 bytes
    ws = [e + e + eu, clef + clef, e + e + clef, eu * 3, clef * 4, clef * 3 + eu + e, eu * 5 + e]
    assert [len(w) for w in ws] == [7, 8, 8, 9, 16, 17, 17]
    return ws


def long_twin_words():
    """same first 8 bytes, same length; the last byte (or 0x00 / 0x80 in it) alone tells them apart"""
    out = []
    for n in (9, 10, 16, 17, 40):
        stem = b"prefix88" + bytes((i * 5 + 65) % 256 for i in range(n - 9))
        stem = stem.replace(b"/", b"_")
        out += [stem + b"x", stem + b"y", stem + b"\x00", stem + b"\x80"]
    out += [b"prefix88\x00tail", b"prefix88\x80tail"]   # ... or a byte in the middle
    return out


def length_words():
    """251-253 bytes with a common 251-byte stem, 254-257 bytes with a common 254-byte stem"""
    a, b = _LONG[:251], bytes(reversed(_LONG[:254]))
    return [a, a[:250] + b"\x80", a + b"q", a + b"qq", b, b + b"q", b + b"qq", b + b"qqq", b + b"qq\x80"]


def vocabulary():
    """every word once, in a fixed order"""
    seen, out = set(), []
    for w in one_byte_words() + nul_words() + twin_words() + utf8_words() + long_twin_words() + length_words():
        assert b"/" not in w and w not in (b"+", b"#")
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def short_vocabulary():
    """the words of at most 40 bytes (random key sets that are compared word by word in Python)"""
    return [w for w in vocabulary() if len(w) <= 40]


def full_range_values(r, n):
    """n distinct u32 values from random.Random r: the edges of the signed range,
    0 and 0xFFFFFFFE first, the rest uniform over [0, 0xFFFFFFFE] (0xFFFFFFFF is
    the library's padding / 'none' value)"""
    vals = [0, 1, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFD]
    seen = set(vals)
    while len(vals) < n:
        v = r.randrange(0, 0xFFFFFFFF)
        if v not in seen:
            seen.add(v)
            vals.append(v)
    return vals[:n]
