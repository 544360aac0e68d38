"""CPU checks of the decode sampler's ground truth: the Philox4x32-10 restatement against Random123's known answers, the reference
kept set (tests/sampling_ref.py) against transformers' own logits processors, and the sampler's C ABI in header and library."""
import itertools
import os
import subprocess

import numpy as np
import pytest
import torch

from myriad_amd import _lib
from tests import sampling_ref as S


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox4x32_10_known_answers(ctr, key, want):
    assert S.philox4x32_10(ctr, key) == want


def test_uniform_is_24_bits_of_the_first_word():
    x0 = S.philox4x32_10((3, 0, 5, 0), (0x12345678, 0x9ABCDEF0))[0]
    u = S.uniform(0x9ABCDEF012345678, 3, 5)
    assert u == (x0 >> 8) / 16777216.0 and 0.0 <= u < 1.0


def _hf_kept(rows, seen, penalty, ban, T, top_k, top_p):
    tr = pytest.importorskip("transformers")
    scores = rows.clone()
    L = len(seen[0])
    input_ids = torch.tensor(seen, dtype=torch.long).reshape(rows.shape[0], L)
    procs = []
    if penalty != 1.0:
        procs.append(tr.RepetitionPenaltyLogitsProcessor(penalty))
    if ban >= 0:
        procs.append(tr.MinLengthLogitsProcessor(L + 1, eos_token_id=ban))
    if T != 1.0:
        procs.append(tr.TemperatureLogitsWarper(T))
    if top_k:
        procs.append(tr.TopKLogitsWarper(top_k))
    if top_p < 1.0:
        procs.append(tr.TopPLogitsWarper(top_p))
    for p in procs:
        scores = p(input_ids, scores)
    return torch.isfinite(scores)


@pytest.mark.parametrize("ties", [False, True])
def test_reference_kept_set_equals_transformers_processors(ties):
    g = torch.Generator().manual_seed(11 if ties else 7)
    R, V, ban = 6, 997, 2
    checked = near = 0
    for top_k, top_p, T, pen, use_ban in itertools.product((1, 7, 50, 400), (0.05, 0.5, 0.9, 1.0), (0.7, 1.0, 1.3), (1.0, 1.3),
                                                           (False, True)):
        x = torch.randn(R, V, generator=g) * 3.0
        if ties:                                   # bf16-quantised, few distinct values: many exact ties at the cuts
            x = (x * 0.5).to(torch.bfloat16).float()
        seen = torch.randint(0, V, (R, 5), generator=g).tolist()
        hf = _hf_kept(x, seen, pen, ban if use_ban else -1, T, top_k, top_p)
        for r in range(R):
            row = S.penalize(x[r], seen[r], pen)
            ref = S.sample_row(row, top_k, top_p, 1.0 / T, ban if use_ban else -1)
            if ref["near"]:
                near += 1
                continue
            assert ref["kept"] == int(hf[r].sum()), (top_k, top_p, T, pen, use_ban, r)
            mine = ref["order"][:ref["kept"]]
            theirs = torch.nonzero(hf[r]).flatten().numpy()
            # tied logits straddling the top-p cut may be kept in either order: compare the kept values (equal as multisets),
            # and the ids exactly whenever the value at the cut is not tied
            assert np.array_equal(np.sort(row[mine].numpy()), np.sort(row[theirs].numpy()))
            if not ties:
                assert set(mine.tolist()) == set(theirs.tolist())
            checked += 1
    assert checked > 0.9 * (checked + near)


def test_sampler_is_declared_and_exported():
    sigs = _lib.parse_header()
    for name in ("mh_sample_rows", "mh_repetition_penalty_rows", "mh_decode_advance_kept"):
        assert name in sigs, name
    assert len(sigs["mh_sample_rows"][1]) == 15 and len(sigs["mh_repetition_penalty_rows"][1]) == 8
    if not os.path.exists(_lib.LIB_PATH):
        from myriad_amd.build import build
        build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T mh_" in ln}
    assert {"mh_sample_rows", "mh_repetition_penalty_rows", "mh_decode_advance_kept"} <= exported
