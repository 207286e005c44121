"""Corrupt copies of user files for the loaders (test_host_mirror.test_decoders_survive_corrupt_files; tools/host_sanitize.py runs the
same mutants through a sanitizer build of the CPU half of the host mirror)."""


def mutate_bytes(rng, base):
    """One mutant of a binary file: one to five of byte overwrite, bit flip, truncation, stray marker (0xFF 0xC0..0xDF)."""
    d = bytearray(base)
    for _ in range(int(rng.integers(1, 6))):
        k = int(rng.integers(0, 4)); p = int(rng.integers(0, len(d)))
        if k == 0: d[p] = int(rng.integers(0, 256))
        elif k == 1: d[p] ^= 1 << int(rng.integers(0, 8))
        elif k == 2 and len(d) > 16: del d[len(d) - int(rng.integers(0, len(d) // 2)):]
        else:
            d[p] = 0xFF
            if p + 1 < len(d): d[p + 1] = 0xC0 + int(rng.integers(0, 32))
    return bytes(d)


_TOKENS = ("0", "-1", "9", "99999999999", "-99999999999", "1e39", "nan", "inf", "", "x", "1/", "/1", "1//", "1/2/3/4", "//", "-0")


def mutate_lines(rng, text):
    """One mutant of a text file of statements (OBJ): one to four of line dropped, doubled, moved, cut short, one token replaced."""
    lines = text.split("\n")
    for _ in range(int(rng.integers(1, 5))):
        k = int(rng.integers(0, 5)); p = int(rng.integers(0, len(lines)))
        if k == 0 and len(lines) > 1: del lines[p]
        elif k == 1: lines.insert(int(rng.integers(0, len(lines) + 1)), lines[p])
        elif k == 2: lines.insert(int(rng.integers(0, len(lines))), lines.pop(p))
        elif k == 3: lines[p] = lines[p][:int(rng.integers(0, len(lines[p]) + 1))]
        else:
            words = lines[p].split(" ")
            words[int(rng.integers(0, len(words)))] = _TOKENS[int(rng.integers(0, len(_TOKENS)))]
            lines[p] = " ".join(words)
    return "\n".join(lines)
