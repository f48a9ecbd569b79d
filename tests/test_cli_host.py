"""epos_amd/cli.py on the CPU: the three scripts' parsers against the snapshot of their flags
(tests/golden/cli_flags.json, written by tests/golden/make_cli_flags.py), the crop-size
parser, the metadata-only frames of a --frames directory and the model-store error."""
import argparse
import builtins
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

from epos_amd import cli   # noqa: E402


def _generator():
  spec = importlib.util.spec_from_file_location(
      'make_cli_flags', os.path.join(GOLDEN, 'make_cli_flags.py'))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


@pytest.mark.parametrize('script', ['infer', 'eval', 'eval_poses'])
def test_parser_flags_match_the_snapshot(script, monkeypatch):
  """(option_strings, dest, default, type name, choices, required, help) of every action, in
  parser order."""
  monkeypatch.delenv('EPOS_LAUNCH_QUEUE', raising=False)   # --launch_queue's default reads it
  with open(os.path.join(GOLDEN, 'cli_flags.json')) as f:
    want = json.load(f)[script]
  got = json.loads(json.dumps(_generator().all_flags()[script]))
  assert len(got) == len(want)
  for g, w in zip(got, want):
    assert g == w


def test_crop_size_spellings():
  for value in ('640,480', [640, 480], (640, 480)):
    assert cli.crop_size(value) == (640, 480)
  assert cli.crop_size('[720, 540]') == (720, 540)


def test_result_suffix_and_model_dir(monkeypatch):
  assert cli.result_suffix(None) == '' and cli.result_suffix('run') == '_run'
  monkeypatch.setenv('TF_MODELS_PATH', '/models')
  assert cli.model_dir(argparse.Namespace(model='m')) == os.path.join('/models', 'm')
  monkeypatch.setenv('EPOS_FORCE_DEVICE', '0')
  assert cli.device_from_env(3) == 0
  monkeypatch.delenv('EPOS_FORCE_DEVICE')
  assert cli.device_from_env(3) == 3 and cli.device_from_env() == 0


def test_metadata_only_frames_open_nothing_but_frames_json(tmp_path, monkeypatch):
  pose = {'obj_id': 2, 'R': np.eye(3).reshape(-1).tolist(), 't': [0.0, 0.0, 500.0]}
  K = [[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]]
  meta = [{'path': 'missing_%d.npy' % i, 'scene_id': 3, 'im_id': i, 'K': K,
           'targets': {'2': 1}, 'gt_poses': [pose]} for i in range(2)]
  meta.append({'im_id': 2, 'K': K})                      # no path, no targets, no poses
  with open(str(tmp_path / 'frames.json'), 'w') as f:
    json.dump(meta, f)
  import epos_amd.dist, epos_amd.frames   # noqa: F401,E401 (before open() is watched)
  opened = []
  real_open = builtins.open

  def recording_open(path, *a, **kw):
    opened.append(str(path))
    return real_open(path, *a, **kw)
  monkeypatch.setattr(builtins, 'open', recording_open)
  monkeypatch.setattr(np, 'load', lambda *a, **kw: pytest.fail('np.load(%r)' % (a,)))
  frames, h, w = cli.load_frames(None, str(tmp_path), 0, '640,480', 480, 0, 0, pixels=False)
  monkeypatch.undo()
  assert opened == [str(tmp_path / 'frames.json')]
  assert (h, w) == (480, 640) and [f.im_id for f in frames] == [0, 1, 2]
  assert frames[0].scene_id == 3 and frames[0].targets == {2: 1}
  assert frames[0].K[0, 2] == 320.0 and frames[1].gt_poses[0]['t'].shape == (3, 1)
  assert frames[2].scene_id == 0 and frames[2].targets == {} and frames[2].gt_poses is None
  assert frames[2].image_path == ''
  # with pixels the same entries need their image files
  with pytest.raises((IOError, OSError)):
    cli.load_frames(None, str(tmp_path), 0, '640,480', 480, 0, 0, meta=meta[:2])
  # entries read by the caller are not read again
  os.remove(str(tmp_path / 'frames.json'))
  again = cli.load_frames(None, str(tmp_path), 0, '640,480', 480, 0, 0, pixels=False,
                          meta=meta)[0]
  assert [f.im_id for f in again] == [0, 1, 2]


def test_load_frames_without_input_raises():
  with pytest.raises(ValueError, match='No input files: give --infer_tfrecord_names'):
    cli.load_frames(None, None, 0, '640,480', 480, 0, 3)
  with pytest.raises(ValueError, match='No input files: .*nowhere.tfrecord'):
    cli.load_frames('nowhere', None, 0, '640,480', 480, 0, 3)
  frames, h, w = cli.load_frames(None, None, 5, [128, 96], 480, 0, 3, rank=1, world=2)
  assert (h, w) == (96, 128) and [f.im_id for f in frames] == [3, 4]


def test_resolve_store_error_text(tmp_path, monkeypatch):
  monkeypatch.delenv('BOP_PATH', raising=False)
  args = argparse.Namespace(num_frags=64, synthetic=0, dataset=None)
  with pytest.raises(ValueError) as e:
    cli.resolve_store(str(tmp_path), args, 3, 'cuda:0')
  assert str(e.value) == ('fragments.pkl / fragments.npz not found in ' + str(tmp_path) +
                          ' and no BOP models under $BOP_PATH/<dataset>/models*')
  # --synthetic: a seeded synthetic store stands in
  args.synthetic = 2
  store = cli.resolve_store(str(tmp_path), args, 3, 'cuda:0')
  assert store.dp_model['obj_ids'] == [1, 2, 3] and store.frag_centers[1].shape == (64, 3)
  # the folder's fragments win over both
  np.savez(str(tmp_path / 'fragments.npz'), obj_ids=np.array([4]),
           frag_centers=np.zeros((1, 64, 3)), frag_sizes=np.ones((1, 64)))
  assert cli.resolve_store(str(tmp_path), args, 3, 'cuda:0').dp_model['obj_ids'] == [4]
