"""CPU-side checks of the predecessor envs' closed-loop rollout (no GPU needed; q3_rollout_policy's declaration and binding are pinned
in tests/abi_table.py and tests/test_abi_host.py): the policy / PPO kernels know the observation length 16 (on a box without a GPU
the create calls get as far as the device check instead of refusing the length); and a null env is refused with a message."""
import ctypes as C


def _lib_and_handle():
    from optimal_quad_control_rl_amd import _lib, build

    build.build_native()
    return _lib, _lib.load()


def test_obs_len_16_is_a_legal_length_and_23_is_not():
    _lib, L = _lib_and_handle()
    h = C.c_void_p()
    # qr_policy_create refuses an illegal length before it looks at the device, on any box; the text names the q3 length too
    assert L.qr_policy_create(23, 0, C.byref(h)) == _lib.QR_E_INVALID
    assert b"or 16" in L.qr_last_error()
    # 16 passes the length check: without a GPU the call gets as far as the device check (QR_E_NO_DEVICE), with one it succeeds
    for create, destroy in ((lambda: L.qr_policy_create(16, 0, C.byref(h)), L.qr_policy_destroy),
                            (lambda: L.qr_ppo_create(16, 0, 4096, C.byref(h)), L.qr_ppo_destroy),
                            (lambda: L.qr_policy_bank_create(16, 0, 2, C.byref(h)), L.qr_policy_bank_destroy)):
        rc = create()
        assert rc in (_lib.QR_OK, _lib.QR_E_NO_DEVICE), (rc, L.qr_last_error())
        if rc == _lib.QR_OK:
            # ... and where there is a device, qr_ppo_create (which looks at the device first) still refuses 23
            assert L.qr_ppo_create(23, 0, 4096, C.byref(C.c_void_p())) == _lib.QR_E_INVALID
            destroy(h)


def test_null_env_is_refused_with_a_message():
    _lib, L = _lib_and_handle()
    ls = (C.c_float * 4)(0, 0, 0, 0)
    rc = L.q3_rollout_policy(None, None, 1, ls, 0, 0, 0, None, None, None, None, None, None, None, None, None, None)
    assert rc == _lib.QR_E_INVALID
    msg = L.qr_last_error()
    assert b"q3_rollout_policy" in msg and b"null" in msg
    assert L.q3_episode_counts(None, None, None, None) == _lib.QR_E_INVALID
