"""Python model of the bench fixture's device calls (include/chunkfs_amd.h,
"Bench fixture"), written for this repository on files_model.Files.

get_to_dedup_ratio is restated twice: `transcription` follows the reference
line by line (src/system/file_layer.rs:212-268: zip with skip(1), unique_by,
take / cycle / take_while, chain with skip), and `closed_form` is the
arithmetic the device uses in its place.  tests/test_bench_model.py holds the
two against each other.  size_distribution and verify restate
CDCFixture::size_distribution and ::verify (src/bench/mod.rs:218-275).
"""
import itertools
import math

import numpy as np

import files_model as fm

EINVAL = -1
U64_MAX = (1 << 64) - 1


def as_usize(x):
    """Rust's `f64 as usize`: truncates, saturates, NaN -> 0."""
    if math.isnan(x):
        return 0
    if x >= 18446744073709551616.0:
        return U64_MAX
    return max(int(x), 0)


def name_of(name, ratio):
    """format!("{name}.{dedup_ratio:.2}")."""
    return "%s.%.2f" % (name, ratio)


def unique_spans(spans):
    """file_layer.rs:225-231: (span, next offset - own offset) over all but the
    last span, the first occurrence of each hash, in file order."""
    seen, out = set(), []
    for first, second in zip(spans, spans[1:]):
        if first.hash in seen:
            continue
        seen.add(first.hash)
        out.append((first, second.offset - first.offset))
    return out


def sizes(lengths, ratio):
    """(total_size, num_repeating) of file_layer.rs:233-237, in f64 as written there."""
    unique_length = sum(lengths)
    total_size = as_usize(float(unique_length) * ratio)
    num_repeating = as_usize(math.ceil(float(len(lengths)) * (1.0 / ratio)))
    return total_size, num_repeating


def never_ends(lengths, ratio):
    """The reference's take_while never fails: it cycles over entries that hold no byte."""
    _, r = sizes(lengths, ratio)
    return r >= 1 and len(lengths) >= 1 and sum(lengths[:r]) == 0


def transcription(unique, ratio):
    """file_layer.rs:233-257 on the unique list [(item, length)]: the items of the new file."""
    lengths = [ln for _, ln in unique]
    if never_ends(lengths, ratio):  # detected, not run
        raise fm.ModelError(EINVAL)
    total_size, num_repeating = sizes(lengths, ratio)
    to_add = [0]

    def within(entry):
        to_add[0] += entry[1]
        return to_add[0] <= total_size

    repeating = itertools.takewhile(within, itertools.cycle(unique[:num_repeating]))
    remaining = unique[num_repeating:]
    return [item for item, _ in itertools.chain(repeating, remaining)]


def closed_form(lengths, ratio):
    """The same as indices into the unique list: K = q * R + j repeating spans
    (span i is entry i mod R), then the entries from R on."""
    if never_ends(lengths, ratio):
        raise fm.ModelError(EINVAL)
    u = len(lengths)
    total_size, r = sizes(lengths, ratio)
    r = min(r, u)
    k = 0
    if r:
        prefix = [0]
        for ln in lengths[:r]:
            prefix.append(prefix[-1] + ln)
        c = prefix[r]
        q, rem = divmod(total_size, c)
        j = max(i for i in range(r + 1) if prefix[i] <= rem)  # entries of length 0 count
        k = q * r + j
    return [i % r for i in range(k)] + list(range(r, u))


def get_to_dedup_ratio(files, name, ratio):
    """FileLayer::get_to_dedup_ratio on a files_model.Files; returns the new
    name.  Offsets in the new file are true byte positions (the layer's one
    deviation; the reference clones the source's offsets)."""
    if not ratio >= 1.0 or math.isinf(ratio):  # NaN and inf: this layer's own refusals
        raise fm.ModelError(EINVAL)
    if name not in files.files:
        raise fm.ModelError(fm.ENOTFOUND)
    picked = transcription(unique_spans(files.files[name]), ratio)
    spans, at = [], 0
    for sp in picked:
        spans.append(fm.Span(sp.hash, at, sp.len))
        at += sp.len
    new_name = name_of(name, ratio)
    files.files[new_name] = spans
    return new_name


def size_distribution(lengths, adjustment):
    """{length // adjustment * adjustment: count}; adjustment 0 divides by zero in the reference."""
    if adjustment == 0:
        raise fm.ModelError(EINVAL)
    out = {}
    for ln in lengths:
        key = int(ln) // adjustment * adjustment
        out[key] = out.get(key, 0) + 1
    return out


def verify(file_bytes, data):
    """(equal, first_diff): the smallest differing offset, min of the sizes
    when only the sizes differ, None when equal."""
    a, b = np.asarray(file_bytes, dtype=np.uint8), np.asarray(data, dtype=np.uint8)
    common = min(a.size, b.size)
    bad = np.nonzero(a[:common] != b[:common])[0]
    if bad.size:
        return False, int(bad[0])
    if a.size != b.size:
        return False, common
    return True, None
