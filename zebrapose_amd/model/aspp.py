"""ASPP + upsampling decoder -- module tree of reference ``zebrapose/model/aspp.py``.

``ASPP`` (:5-114, 512-channel input), ``ASPP_50`` (:117-225, 2048-channel input) and
``ASPP_non_binary_ablationstudy`` (:228-340, the d-ary code head pair) with the reference's
attribute names; ``upsample()`` returns the same 9-entry
Sequential (ConvT, BN, ReLU, conv3x3, BN, ReLU, conv3x3, BN, ReLU; :60-80).
The computation is done by ``zebrapose_amd.engine``.
"""
from __future__ import annotations

import torch.nn as nn

from .layers import AdaptiveAvgPool2d, BatchNorm2d, Conv2d, ConvTranspose2d, ReLU


def _upsample(in_channels, num_filters, kernel_size=3, padding=1, output_padding=1):
    return nn.Sequential(
        ConvTranspose2d(in_channels, num_filters, kernel_size=kernel_size, stride=2, padding=padding,
                        output_padding=output_padding, bias=False),
        BatchNorm2d(num_filters), ReLU(inplace=True),
        Conv2d(num_filters, num_filters, kernel_size=3, stride=1, padding=1, bias=False),
        BatchNorm2d(num_filters), ReLU(inplace=True),
        Conv2d(num_filters, num_filters, kernel_size=3, stride=1, padding=1, bias=False),
        BatchNorm2d(num_filters), ReLU(inplace=True))


class _ASPPBase(nn.Module):
    in_high = 512
    x64_channels = 64

    def __init__(self, num_classes, concat=True, output_kernel_size=1):
        super().__init__()
        self.num_classes = num_classes
        pad = self._trunk(concat, output_kernel_size)
        self.conv_1x1_4 = Conv2d(256 + 64, num_classes, kernel_size=output_kernel_size, padding=pad)

    def _trunk(self, concat, output_kernel_size):
        """Everything up to the head conv(s), in the reference's registration order; returns the
        head's padding."""
        if output_kernel_size not in (1, 3):
            raise NotImplementedError("output_kernel_size must be 1 or 3")
        self.concat = concat
        self.output_kernel_size = output_kernel_size
        c = self.in_high
        self.conv_1x1_1 = Conv2d(c, 256, kernel_size=1)
        self.bn_conv_1x1_1 = BatchNorm2d(256)
        self.conv_3x3_1 = Conv2d(c, 256, kernel_size=3, stride=1, padding=6, dilation=6)
        self.bn_conv_3x3_1 = BatchNorm2d(256)
        self.conv_3x3_2 = Conv2d(c, 256, kernel_size=3, stride=1, padding=12, dilation=12)
        self.bn_conv_3x3_2 = BatchNorm2d(256)
        self.conv_3x3_3 = Conv2d(c, 256, kernel_size=3, stride=1, padding=18, dilation=18)
        self.bn_conv_3x3_3 = BatchNorm2d(256)
        self.avg_pool = AdaptiveAvgPool2d(1)
        self.conv_1x1_2 = Conv2d(c, 256, kernel_size=1)
        self.bn_conv_1x1_2 = BatchNorm2d(256)
        self.conv_1x1_3 = Conv2d(1280, 256, kernel_size=1)
        self.bn_conv_1x1_3 = BatchNorm2d(256)
        if concat:
            self.upsample_1 = self.upsample(256, 256, 3, 1, 1)
            self.upsample_2 = self.upsample(256 + self.x64_channels, 256, 3, 1, 1)
        else:
            self.upsample_1 = self.upsample(256, 256, 3, 1, 1)
            self.upsample_2 = self.upsample(256, 256, 3, 1, 1)
        return 1 if output_kernel_size == 3 else 0

    def upsample(self, in_channels, num_filters, kernel_size, padding, output_padding):
        return _upsample(in_channels, num_filters, kernel_size, padding, output_padding)


class ASPP(_ASPPBase):
    """aspp.py:5-114 (ResNet34 encoder, 512-channel high feature, 64-channel x_64 skip)."""
    in_high = 512
    x64_channels = 64


class ASPP_50(_ASPPBase):
    """aspp.py:117-225 (ResNet50 encoder, 2048-channel high feature, 256-channel x_64 skip)."""
    in_high = 2048
    x64_channels = 256


class ASPP_non_binary_ablationstudy(_ASPPBase):
    """aspp.py:228-340 (ResNet34 encoder): ASPP's trunk with two head convs over the 320-channel
    [up2 | x_128] concat, ``conv_1x1_4_mask`` (-> 1) and ``conv_1x1_4_code`` (-> L * d: L groups of d
    class logits, aspp.py:281-282, 337-338)."""
    in_high = 512
    x64_channels = 64

    def __init__(self, code_output_length=16, divided_number_each_iteration=2, concat=True,
                 decoder_last_layer_also_concat=False, output_kernel_size=1):
        nn.Module.__init__(self)
        self.decoder_last_layer_also_concat = decoder_last_layer_also_concat
        self.code_output_length = code_output_length
        self.divided_number_each_iteration = divided_number_each_iteration
        pad = self._trunk(concat, output_kernel_size)
        self.conv_1x1_4_mask = Conv2d(256 + 64, 1, kernel_size=output_kernel_size, padding=pad)
        self.conv_1x1_4_code = Conv2d(256 + 64, code_output_length * divided_number_each_iteration,
                                      kernel_size=output_kernel_size, padding=pad)
