"""Plain NumPy restatement of the black box's bookkeeping (qr_blackbox_policy, csrc/quadrace_blackbox.hip; contract in include/quadrace.h).
Test infrastructure: the GPU tests record the same flight with qr_record_policy on a twin handle, feed those rows [K][M][R] through
`run()` / `run_arrays()` below and demand that the kernel's ring and status are EQUAL.  Nothing here is arithmetic on floats: rows are copied.

Per env: a row of call-step k goes to ring slot (first_step + k) mod W iff the env was armed at the START of the step; the env freezes
at the end of a step whose end code (column S + 5: 1 crash, 2 time limit) has its bit in `trigger`.  Status, 4 int32:
    0 armed (0) / frozen (1)     1 rows stored so far (cumulative)     2 ring slot of the trigger row, -1 while armed     3 cause bits
The cause bits come from the terminal state, which recorder rows do not hold: `run()` leaves [3] of a newly frozen env at 0 and reports
which envs it froze, and `cause_bits()` restates the comparisons on a terminal state.
"""
import numpy as np

ST_INTS = 4
ON_CRASH, ON_TIME_LIMIT = 1, 2
CAUSE_GROUND, CAUSE_OOB, CAUSE_TIME_LIMIT, CAUSE_GATE = 1, 2, 4, 8


def new_status(m):
    return np.zeros((m, ST_INTS), np.int32)


def run_arrays(rows, first_step, window, trigger, status=None):
    """The bookkeeping on arrays.  rows [K][M][R] float32 (recorder rows of call-steps 0..K-1), status [M][4] or None (fresh).
    Returns (source, status, trigger_step): source [W][M] = the call-step whose row this call left in that slot (the last write wins),
    -1 for a slot this call did not write; the new status; trigger_step [M] = the call-step at which env i froze in THIS call, or -1."""
    rows = np.asarray(rows)
    K, M, R = rows.shape
    s, w = R - 8, int(window)
    st = new_status(M) if status is None else np.array(status, np.int32, copy=True)
    armed_at_entry = st[:, 0] == 0
    st[armed_at_entry, 2] = -1          # a zeroed status is a fresh one
    st[armed_at_entry, 3] = 0
    source = np.full((w, M), -1, np.int64)
    trigger_step = np.full(M, -1, np.int64)
    for k in range(K):
        slot = (int(first_step) + k) % w
        armed = st[:, 0] == 0                                            # at the START of the step: the triggering row is stored
        source[slot, armed] = k
        st[armed, 1] += 1
        code = rows[k, :, s + 5].astype(np.int64)
        hit = armed & (code != 0) & ((code & int(trigger)) != 0)          # end codes 1 and 2 are their own trigger bits
        st[hit, 0], st[hit, 2] = 1, slot
        trigger_step[hit] = k
    return source, st, trigger_step


def run(rows, first_step, window, trigger, status=None):
    """As run_arrays, with the ring as a dict of written slots per env: written[i] = {slot: row}."""
    rows = np.asarray(rows)
    source, st, trigger_step = run_arrays(rows, first_step, window, trigger, status)
    written = [{int(slot): rows[source[slot, i], i] for slot in np.nonzero(source[:, i] >= 0)[0]} for i in range(rows.shape[1])]
    return written, st, trigger_step


def ring_from_source(rows, source, fill):
    """The ring [W][M][R] that a buffer holding `fill` (a scalar or a [W][M][R] array: the ring before the call) holds afterwards."""
    rows = np.asarray(rows)
    w, m = source.shape
    ring = np.array(np.broadcast_to(np.asarray(fill, np.float32), (w, m, rows.shape[2])), np.float32, copy=True)
    sl, en = np.nonzero(source >= 0)
    ring[sl, en] = rows[source[sl, en], en]
    return ring


def cause_bits(term, end_code):
    """Cause bits of one env from its terminal world state `term` [S] (float32) and the end code of the trigger row: the comparisons of
    the env step, on the state after the integration."""
    t = np.asarray(term, np.float32)
    ground = bool(t[2] > 0.0)
    oob = bool(abs(t[0]) > 10.0 or abs(t[1]) > 10.0 or abs(t[9]) > 1000.0 or abs(t[10]) > 1000.0 or abs(t[11]) > 1000.0)
    trunc = int(end_code) == 2
    return (CAUSE_GROUND if ground else 0) | (CAUSE_OOB if oob else 0) | (CAUSE_TIME_LIMIT if trunc else 0) | \
        (CAUSE_GATE if (not trunc and not ground and not oob) else 0)


def valid_slots(status_row, first_step, num_steps, window):
    """Ring slots of env i's valid rows, oldest first: min(st[1], W) rows that end at st[2] if frozen, at the call's last slot if armed."""
    n = int(min(status_row[1], window))
    end = int(status_row[2]) if status_row[0] else int((int(first_step) + int(num_steps) - 1) % int(window))
    return [(end - n + 1 + j) % int(window) for j in range(n)]
