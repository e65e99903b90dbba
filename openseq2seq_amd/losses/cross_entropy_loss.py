"""CrossEntropyLoss — open_seq2seq/losses/cross_entropy_loss.py: tf.losses.softmax_cross_entropy of one-hot (any
dense) labels, the per-sample -sum_c y_c log softmax(logits)_c summed and divided by the batch size. One launch
(os2s_softmax_xent_dense, csrc/text_cls.hip) writes the fp32 loss and, in training, d(logits) times the device loss
scale. Logits [B, C] fp32 with 2 <= C <= 16: the text-classification head of LSTMLM."""
from __future__ import absolute_import, division, print_function

import torch

from .loss import Loss
from .. import capi


class CrossEntropyLoss(Loss):
  def __init__(self, params, model, name="cross_entropy_loss"):
    super(CrossEntropyLoss, self).__init__(params, model, name)

  def _compute_loss(self, input_dict):
    dec = input_dict['decoder_output']
    logits = dec['logits']
    if logits.dim() != 2 or logits.dtype != torch.float32 or not 2 <= logits.shape[1] <= 16:
      raise NotImplementedError("CrossEntropyLoss on %s %s logits (built for the [B, C <= 16] fp32 logits of the "
                                "text-classification head)" % (tuple(logits.shape), logits.dtype))
    labels = input_dict['target_tensors'][0].to(torch.float32).contiguous()
    la = dec.get('logits_act')
    want_grad = la is not None and input_dict.get('want_grad', True)
    loss, dl = capi.softmax_xent_dense(logits, labels, grad_scale_dev=input_dict.get('loss_scale_dev'),
                                       want_grad=want_grad)
    if want_grad:
      la.grad = dl
      la.grad_init = True
    return loss
