"""train_episodes(..., render_dir=...) (antsrl_amd/driver.py): ReworkAgent, 3 episodes of 6 steps, 3 environments of 64
ants, snapshot_every = 2 (episodes 0 and 1 are visualised), render_every = 2.  The PNG files it writes — episode_%04d/
frame_%05d.png for frames 0, 2 and 4 of the visualised episodes, and no others — decode to the bytes render() gives for
the same run recorded by hand and to the bytes of tests/render_ref.py; the run's statistics are those of the run without
render_dir; and render_dir without snapshot_on_device is refused."""
import os

import numpy as np
import pytest

import monitor_ref as R
import render_ref as RR
from agent_harness import make_env

pytestmark = pytest.mark.gpu

E, N, STEPS, EPISODES, SEED = 3, 64, 6, 3, 21


def the_gen():
    from antsrl_amd import config as cm
    return cm.make_gen(wall_density=0.05, n_food_discs=6, food_rmin=3, food_rmax=6)


def make_agent():
    from antsrl_amd.agent import ReworkAgent
    return ReworkAgent(epsilon=0.5, learning_rate=1e-3, min_replay=300, replay_size=3000, minibatch=64, seed=7)


def test_the_pngs_decode_to_the_bytes_of_render(tmp_path, monkeypatch):
    from PIL import Image
    from antsrl_amd import snapshot
    from antsrl_amd.driver import train_episodes
    from antsrl_amd.render import EpisodeRenderer
    kept = []
    save = EpisodeRenderer.save

    def keeping(self, directory, **kw):  # what render() and the recorder held at the moment the files were written
        kept.append((directory, self.zoom, self.ant_radius, self.render()[:, 0].cpu().numpy(), self.rec.frames()))
        return save(self, directory, **kw)
    monkeypatch.setattr(EpisodeRenderer, "save", keeping)
    out = str(tmp_path / "pictures")
    log = train_episodes(make_agent(), make_env(E, N, STEPS), the_gen(), EPISODES, STEPS, seed=SEED, snapshot_every=2,
                         snapshot_on_device=True, snapshot_envs=(1, 0), render_dir=out, render_every=2)
    assert sorted(os.listdir(out)) == ["episode_0000", "episode_0001"] and len(kept) == 2
    for (directory, zoom, ra, frames, f), episode in zip(kept, (0, 1)):
        assert directory == os.path.join(out, "episode_%04d" % episode)
        assert sorted(os.listdir(directory)) == ["frame_%05d.png" % k for k in (0, 2, 4)]
        assert (zoom, ra) == (8, 4) and frames.shape == (STEPS, 64 * 8, 64 * 8, 3)
        want = RR.render_frames(f, 0, STEPS, snapshot.PHERO_COLORS[:2], 255.0, zoom, RR.VIEW_ALL, ra)[:, 0]
        assert np.array_equal(frames, want)
        for k in (0, 2, 4):
            png = np.asarray(Image.open(os.path.join(directory, "frame_%05d.png" % k)).convert("RGB"))
            assert png.dtype == np.uint8 and np.array_equal(png, frames[k]), (episode, k)
    assert not np.array_equal(kept[0][3], kept[1][3])
    # drawing perturbs nothing: the same run without render_dir
    plain = train_episodes(make_agent(), make_env(E, N, STEPS), the_gen(), EPISODES, STEPS, seed=SEED, snapshot_every=2,
                           snapshot_on_device=True, snapshot_envs=(1, 0))
    assert snapshot.dumps(log["states"]) == snapshot.dumps(plain["states"])
    for k in ("reports", "all_reward", "all_loss", "grand_total", "epsilons"):
        assert np.array_equal(R.bits(log[k]), R.bits(plain[k])), k


def test_render_dir_needs_the_recorder(tmp_path):
    from antsrl_amd.driver import train_episodes
    with pytest.raises(ValueError, match="snapshot_on_device"):
        train_episodes(make_agent(), make_env(E, N, STEPS), the_gen(), 1, STEPS, snapshot_every=1, render_dir=str(tmp_path))
    assert os.listdir(str(tmp_path)) == []
