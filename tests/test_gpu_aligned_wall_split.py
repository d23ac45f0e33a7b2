"""The wall / plane split of a float32 (env, agent) block sits on a 128-byte line of the block's ADDRESS (wall_split_vec in
pmx_device.h): the wall writer (phase A0 of pmx_tick_fused_kernel, write_walls of the rule launch) stores the vectors in front
of it with streaming stores, the expansion behind it (fused_expand_block, pmx_expand_kernel<0, false, true>) everything from
there on, the wall-only vectors up to the end of plane 0 included.  A vector neither side stores, or a split that depends on
anything but the address, shows here as a byte of the prefill pattern left in the caller's buffer.

* every byte on boards of every residue of H*W mod 4, on smallCapture (4 928-byte blocks, bases alternating 0 and 64 mod 128)
  and on the two smallest boards, where the split is 0 for some or all blocks and the wall writer stores nothing for them;
  one-launch and two-launch path, both sweeps, against the full-plane expansion (a twin handle under an open profile, which
  takes pmx_expand_kernel<0, false>), with pmx_observe for the block of agent 3, and canary bands around the buffer;
* the same with the caller's buffer 16, 48 and 80 bytes into an allocation: the result equals that of the aligned buffer;
* per-env layouts on the two-launch path: every env shows its own walls.

(The wall vectors as lane masks in the kernel's arguments were measured and not kept, see profiles/aligned_split/README.md; the
test of the host-built masks went with them.)"""
import functools

import numpy as np
import pytest
import torch

TICKS = 3
BAND = 256                      # canary bytes on either side of the observation buffer
NAN_BYTE, CANARY = 0xFF, 0xA5   # 0xFFFFFFFF is a NaN: no plane element ever holds it

BOARDS = {
    "board8x3": ["%%%%%%%%", "%13..42%", "%%%%%%%%"],                                  # H*W = 24: 6 wall vectors, blocks of 6 lines
    "board9x3": ["%%%%%%%%%", "%13. .42%", "%%%%%%%%%"],                               # 27 (3 mod 4): 6 wall vectors, 6.75 lines
    "board8x5": ["%%%%%%%%", "%1 .. 2%", "%  ..  %", "%3 .. 4%", "%%%%%%%%"],          # 40 (0 mod 4): plane 0 ends on a vector
    "board9x5": ["%%%%%%%%%", "%1 . . 2%", "% .   . %", "%3 . . 4%", "%%%%%%%%%"],     # 45 (1 mod 4)
    "smallCapture": None,                                                              # 154 (2 mod 4)
}
# the splits a 128-byte aligned buffer of >= 8 blocks must show (computed by hand from the block sizes, see _split)
SPLITS = {"board8x3": {0}, "board9x3": {0, 2, 4, 6}, "board8x5": {8}, "board9x5": {4, 6, 8, 10}, "smallCapture": {32, 36}}

_MAZE_A = ["%%%%%%%%%%", "%1 .  . 2%", "% %%  %% %", "%  .  .  %", "% %    % %", "%3 .  . 4%", "%%%%%%%%%%"]
_MAZE_B = ["%%%%%%%%%%", "%1 .  . 2%", "%  %  %  %", "% %.  .% %", "%   %%   %", "%3 .  . 4%", "%%%%%%%%%%"]


def _pmx():
    import pmx
    return pmx


def _layout(board):
    pmx = _pmx()
    return pmx.get_layout(board) if BOARDS[board] is None else pmx.Layout.from_text(BOARDS[board])


def _split(addr, first_vec):
    """wall_split_vec restated: the largest s <= first_vec with addr + 16 s on a 128-byte line, 0 if there is none"""
    for s in range(first_vec, 0, -1):
        if (addr + 16 * s) % 128 == 0:
            return s
    return 0


def test_the_boards_cover_every_residue_and_the_empty_split():
    assert sorted((len(r) * len(r[0])) % 4 for r in (BOARDS[b] or _layout(b).text for b in BOARDS)) == [0, 0, 1, 2, 3]
    for b in BOARDS:
        lay = _layout(b)
        hw = lay.width * lay.height
        assert {_split(q * 32 * hw, hw // 4) for q in range(8)} == SPLITS[b], b
    assert 8 * 3 * 4 // 16 < 8 and 9 * 3 * 4 // 16 < 8            # the two boards with fewer than 8 wall vectors


# ---- every byte ------------------------------------------------------------------------------------------------------------------

def _actions(N, seed):
    rng = np.random.RandomState(seed)
    return [torch.tensor(rng.randint(0, 5, size=(N, 4)).astype(np.int8)) for _ in range(TICKS)]


def _make(layout, N, alt, fused, **kw):
    env = _pmx().PmxVecEnv(layout, N, length=2, auto_reset=True, seed=3, **kw)
    env.set_tuning("expand_alt", alt)
    env.set_tuning("fused_min_envs", 64 if fused else N + 1)
    return env


def _banded(env, offset):
    """env.obs becomes a view `offset` bytes behind a 128-byte line of a larger allocation, canary bands on both sides"""
    n = env.obs.numel() * 4
    raw = torch.empty(BAND + offset + n + BAND + 128, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 128 == 0
    raw.fill_(CANARY)
    env.obs = raw[BAND + offset:BAND + offset + n].view(torch.float32).view(env.obs.shape)
    assert env.obs.data_ptr() % 128 == offset % 128
    return raw


def _prefill(raw, offset, n):
    raw[BAND + offset:BAND + offset + n].fill_(NAN_BYTE)


def _bands_intact(raw, offset, n):
    return bool((raw[:BAND + offset] == CANARY).all()) and bool((raw[BAND + offset + n:] == CANARY).all())


@functools.lru_cache(maxsize=None)
def _full_plane_reference(board, N, alt):
    """per tick: the bytes of the full-plane expansion (a handle under an open profile: rule launch without wall blocks and
    pmx_expand_kernel<0, false>) and pmx_observe's planes of agent 3, whose block shows the tick's final state"""
    env = _make(_layout(board), N, alt, fused=False)
    env.reset()
    env.profile_begin(4 * TICKS)
    out = []
    for a in _actions(N, 77):
        env.obs.fill_(float("nan"))
        obs, *_ = env.step(a.cuda())
        assert not env.last_step_fused()
        step_bytes = obs.view(torch.uint8).cpu().numpy().copy()
        env.obs.fill_(float("nan"))
        seen, _ = env.observe(want_legal=False)
        out.append((step_bytes, seen[:, 3].contiguous().view(torch.uint8).cpu().numpy().copy()))
    prof = env.profile_end()
    assert prof["expand_launches"] >= TICKS
    env.close()
    for step_bytes, agent3 in out:
        assert not np.isnan(step_bytes.view(np.float32)).any()
        assert (step_bytes.reshape(N, 4, -1)[:, 3] == agent3.reshape(N, -1)).all()
    return out


def _run(board, N, alt, fused, offset):
    env = _make(_layout(board), N, alt, fused)
    env.reset()
    n = env.obs.numel() * 4
    raw = _banded(env, offset)
    got = []
    for a in _actions(N, 77):
        _prefill(raw, offset, n)
        obs, *_ = env.step(a.cuda())
        assert env.last_step_fused() == fused
        assert obs.data_ptr() == raw.data_ptr() + BAND + offset
        got.append(obs.view(torch.uint8).cpu().numpy().copy())
        assert _bands_intact(raw, offset, n), "bytes outside the observation buffer were written"
    env.close()
    return got


def _compare(got, ref, tag):
    for t, (g, (want, _)) in enumerate(zip(got, ref)):
        bad = np.argwhere(g.reshape(-1) != want.reshape(-1))
        assert len(bad) == 0, f"{tag} t={t}: {len(bad)} bytes differ from the full-plane expansion, first at byte {int(bad[0])} " \
                              f"(block {int(bad[0]) // (want.size // (want.shape[0] * 4))})"


@pytest.mark.gpu
@pytest.mark.parametrize("alt", [0, -1])
@pytest.mark.parametrize("fused", [True, False], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("board", sorted(BOARDS))
def test_every_byte_on_every_phase_of_alignment(board, fused, alt):
    N = 128                                     # two workgroups of the one-launch kernel
    _compare(_run(board, N, alt, fused, 0), _full_plane_reference(board, N, alt), f"{board} fused={fused} alt={alt}")


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [16, 48, 80])
@pytest.mark.parametrize("fused", [True, False], ids=["one_launch", "two_launches"])
@pytest.mark.parametrize("board", ["board9x3", "smallCapture"])
def test_buffer_base_off_the_128_byte_line(board, fused, offset):
    """the split follows the address: blocks of a shifted buffer split elsewhere, and every byte is still stored once"""
    N = 128
    lay = _layout(board)
    hw = lay.width * lay.height
    assert {_split(offset + q * 32 * hw, hw // 4) for q in range(8)} != SPLITS[board]
    _compare(_run(board, N, -1, fused, offset), _full_plane_reference(board, N, -1), f"{board} fused={fused} +{offset}")


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 48])
def test_per_env_layouts_keep_their_own_walls(offset):
    """two boards of 10 x 7 (2 240-byte blocks: bases alternate 0 and 64 mod 128, splits 16 and 12 of 17 wall vectors) dealt to the
    envs 3 : 1, so that neighbouring blocks differ in layout and in split; the two-launch path recomputes the walls per env"""
    pmx = _pmx()
    N = 96
    lays = [pmx.Layout.from_text(_MAZE_A), pmx.Layout.from_text(_MAZE_B)]
    index = (np.arange(N) % 4 == 3).astype(np.int32)
    assert {_split(q * 2240, 17) for q in range(4)} == {16, 12}
    walls = np.stack([np.array([[float(l.is_wall(x, y)) for x in range(10)] for y in range(7)], np.float32) for l in lays])
    assert (walls[0] != walls[1]).any()
    T = _make(lays, N, -1, fused=False, layout_index=index)
    R = _make(lays, N, -1, fused=False, layout_index=index)
    T.reset()
    R.reset()
    R.profile_begin(4 * TICKS)
    n = T.obs.numel() * 4
    raw = _banded(T, offset)
    for t, a in enumerate(_actions(N, 78)):
        _prefill(raw, offset, n)
        R.obs.fill_(float("nan"))
        got, *_ = T.step(a.cuda())
        want, *_ = R.step(a.cuda())
        assert not T.last_step_fused()
        assert torch.equal(got.view(torch.uint8).cpu(), want.view(torch.uint8).cpu()), f"t={t}"
        assert _bands_intact(raw, offset, n)
        plane0 = got[:, :, 0].cpu().numpy()
        assert (plane0 == walls[index][:, None]).all(), f"t={t}: an env does not show its own walls"
    R.profile_end()
    T.close()
    R.close()
