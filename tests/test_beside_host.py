"""csrc/host/beside.h without a device: tests/cpp/beside_host.cpp, a stand-alone program that defines the five mi_dspu_* functions
the header calls over host memory, built with the address and undefined-behaviour sanitizers and run directly.  It prints one line
per check; what each must say is held here.  A write past a buffer's rows * cap floats, a leak or a double free ends the program
with the sanitizer's report and a non-zero status."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROGRAM = os.path.join(ROOT, "tests", "cpp", "beside_host.cpp")
HOST = os.path.join(ROOT, "lsp-dsp-units_amd", "csrc", "host")


@pytest.fixture(scope="module")
def said(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("beside_host") / "beside_host")
    # the sanitizers' runtimes linked in: the program starts the same whatever libraries its environment loads in front of it
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                           "-I" + os.path.join(ROOT, "include"), "-I" + HOST, PROGRAM, "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert run.returncode == 0, run.stderr.decode()
    return {l.split()[0]: [int(v) for v in l.split()[1:]] for l in run.stdout.decode().splitlines() if l.strip()}


def test_rows_reallocates_only_for_more_floats_or_more_rows(said):
    # per reserve(): ok, allocations so far, cap, rows, bytes of the last allocation
    steps = [said["reserve"][i:i + 5] for i in range(0, 25, 5)]
    assert steps[0] == [1, 1, 4, 2, 4 * 2 * 4]                 # reserve(4, 2)
    assert steps[1] == steps[0] and steps[2] == steps[0]       # reserve(3, 2) and reserve(4, 1) fit
    assert steps[3] == [1, 2, 5, 2, 5 * 2 * 4]                 # reserve(5, 2): longer rows
    assert steps[4] == [1, 3, 4, 3, 4 * 3 * 4]                 # reserve(4, 3): more rows, of the length asked for


def test_row_k_starts_k_capacities_behind_row_0(said):
    assert said["row"] == [0, 4, 8]


def test_up_then_down_gives_back_every_row_and_touches_no_other(said):
    assert said["roundtrip"] == [1, 1]                          # n = 1 and n = cap, three rows of 7


def test_a_failed_allocation_leaves_the_buffer_empty_and_the_next_succeeds(said):
    # live before; then the failed reserve: result, cap, rows, live; then the next: result, cap, rows, live
    assert said["failed"] == [1, 0, 0, 0, 0, 1, 8, 2, 1]


def test_the_destructor_releases_and_an_empty_buffer_has_no_rows(said):
    assert said["destroyed"] == [0]
    assert said["empty"] == [1, 0, 0]
    assert said["live"] == [0]


def test_of_makes_an_entry_once_per_address(said):
    assert said["of_twice"] == [1, 1, 1, 0]                     # the same entry, one make, one construction, none destroyed


def test_a_failing_make_stores_nothing_and_the_next_call_makes_again(said):
    # null, not found, makes, constructed, destroyed (the half-made one, once); then: an entry, makes, constructed, destroyed
    assert said["make_fails"] == [1, 1, 2, 2, 1, 1, 3, 3, 1]


def test_drop_destroys_once_and_ignores_what_it_does_not_know(said):
    assert said["drop"] == [2, 1, 2, 3]                         # destroyed, gone from the table; after two more drops: the same


def test_a_dropped_address_gets_a_new_entry(said):
    assert said["again"] == [4, 4, 4]                           # the fourth make's entry


def test_find_never_makes_an_entry(said):
    assert said["find"] == [1, 1, 0]
    assert said["balance"] == [4, 4, 0]                         # constructed, destroyed, allocations left


def test_four_threads_of_and_drop_on_distinct_addresses(said):
    assert said["threads"] == [0, 0, 4 * 64, 4 * 64, 0]         # wrong answers, entries left, constructed, destroyed, allocations left


def test_beside_destroys_the_bank_it_was_given_and_none_after_a_failed_create(said):
    # channels, equal state not sent, other state sent once, sends, allocations, held word; after drop: created, destroyed,
    # allocations left; a refused create: no entry, no further destroy
    assert said["beside"] == [1, 1, 1, 1, 1, 7, 1, 1, 0, 1, 1]
