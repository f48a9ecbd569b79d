"""SHA-256 of what two training steps on the small net of tests/helpers/loss_device.py leave
behind, in three configurations -- the logits variables only, all nine, the logits variables
plus the layer's weights: after each step every entry of the optimiser's state() and the three
forward_logits tensors. Run from the root of a tree; it uses the names that tree has (the
parent's two optimisers and two train steps, or epos_amd/trainer.py), so that the listing of the
parent commit and of this tree can be compared line by line.

    python profiles/r26/same_bytes.py > listing.txt
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())

from epos_amd import decoder_train, loss, model, synthetic, weights   # noqa: E402
from tests.helpers import loss_cases                                   # noqa: E402
from tests.helpers.loss_device import NET_B, NET_F, NET_H, NET_O, NET_W, gt_tensors  # noqa: E402

try:
  from epos_amd import trainer
except ImportError:
  trainer = None
  from epos_amd import heads_train

LR = 1e-3
KW = dict(momentum=0.9, weight_decay=4e-5, last_layer_gradient_multiplier=3.0)
NINE = loss.HEAD_VARIABLES + decoder_train.LAYER_VARIABLES
CONFIGS = (('logits only', None), ('all nine', NINE),
           ('logits + layer weights', loss.HEAD_VARIABLES + decoder_train.LAYER_VARIABLES[:1]))


def make(ckpt, trainable):
  """(optimiser, train step, update) of a configuration under this tree's names."""
  if trainer is not None:
    opt = trainer.Optimizer(ckpt, LR, trainable=trainable, **KW)
    return opt, trainer.train_step, lambda net, v: net.set_weights(v)
  if trainable is None:
    return (heads_train.HeadsOptimizer(ckpt, LR, **KW), heads_train.train_step,
            lambda net, v: net.set_layer_weights(v))
  return (decoder_train.DecoderOptimizer(ckpt, LR, trainable=trainable, **KW),
          decoder_train.train_step_decoder, lambda net, v: net.set_layer_weights(v))


def sha(a):
  return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
  ckpt = weights.random_init('xception_65', num_objs=NET_O, num_frags=NET_F, seed=5,
                             randomize_bn=True)
  mo = model.ModelOptions(model.get_outputs_to_num_channels(NET_O, NET_F),
                          crop_size=(NET_W, NET_H))
  net = model.get_net(ckpt, NET_B, NET_H, NET_W, NET_O, NET_F, mo, 'cuda:0')
  images = np.stack([synthetic.image(i, NET_H, NET_W) for i in range(NET_B)]).astype(np.float32)
  gt = gt_tensors(loss_cases.make_case(NET_B, net.out_h * net.out_w, NET_O, NET_F, seed=41),
                  net.out_h, net.out_w)
  for tag, trainable in CONFIGS:
    opt, train_step, update = make(ckpt, trainable)
    update(net, {n: np.asarray(ckpt[n]) for n in NINE})       # every configuration starts alike
    for step in range(2):
      values, bad, status = train_step(net, images, gt, opt, LR)
      assert bad.tolist() == [0] * NET_B and not status.any().item()
      print('%s, step %d: values %s' % (tag, step, sha(values.cpu().numpy())))
      for name, v in sorted(opt.state().items()):
        print('%s, step %d: %s %s' % (tag, step, name, sha(v)))
      for name, t in sorted(net.forward_logits(images).items()):
        print('%s, step %d: forward_logits %s %s' % (tag, step, name, sha(t.cpu().numpy())))
  torch.cuda.synchronize()


if __name__ == '__main__':
  main()
