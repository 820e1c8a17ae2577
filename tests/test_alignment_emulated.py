"""CPU: translation alignment on the device (lm_align_*, device.TranslationAligner, the overlay's Aligner) with the kernels
running in the emulated build of the HIP sources; the checks are tests/alignment_checks.py, the same ones
tests/test_alignment_gpu.py runs on the GPU.  The last test runs the reference's own Evaluator over the overlay's Aligner and
needs the reference tree, which only the build container has: it is skipped where the tree is absent."""
import os
import subprocess
import sys

import pytest

import alignment_checks as ac
import lm_checks

sys.path.append(lm_checks.GOLD)
import ref_env  # noqa: E402  (where the reference tree is expected; nothing of it is imported in this process)


def test_fixture_is_not_vacuous():
    ac.check_not_vacuous()


def test_g21_through_the_overlay(emu_lib):
    ac.check_g21_overlay(emu_lib)


def test_g21_counts_against_numpy(emu_lib):
    ac.check_counts_g21(emu_lib)


def test_batch_of_pairs_against_numpy(emu_lib):
    ac.check_batch(emu_lib)


def test_pixel_stride_reads_one_channel_in_place(emu_lib):
    ac.check_pixel_stride(emu_lib)


def test_device_input_equals_host_input(emu_lib):
    ac.check_device_input(emu_lib)


def test_all_ink_closed_form(emu_lib):
    ac.check_all_ink(emu_lib, 9, 70, 9)


def test_empty_image_inside_a_batch(emu_lib):
    ac.check_empty_in_batch(emu_lib)


def test_handle_reuse_leaves_no_stale_bits(emu_lib):
    ac.check_reuse(emu_lib)


def test_argument_checks(emu_lib):
    ac.check_argument_errors(emu_lib)


@pytest.mark.parametrize("name", lm_checks.STREAMS)
def test_keyframes_alignments_parity(emu_lib, name):
    ac.check_keyframes_parity(emu_lib, name)


@pytest.mark.skipif(not ref_env.available(), reason="needs the reference tree")
def test_reference_evaluator_runs_over_the_overlay_aligner(emu_lib):
    """the UNMODIFIED reference Evaluator.keyframes_alignments and Evaluator.parallel_keyframe_align, importing the overlay's module
    as AccessMath.preprocessing.content.aligner, return the recorded tuples (a child process: the reference's packages shadow the
    overlay's there)"""
    src = ac.REFERENCE_CHILD % {"tests": os.path.dirname(os.path.abspath(__file__)), "root": lm_checks.ROOT, "ref": ref_env.REF_ROOT,
                                "lib": emu_lib.path}
    r = subprocess.run([sys.executable, "-c", src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "reference evaluator over the overlay aligner ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
