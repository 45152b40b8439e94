"""Top-level module name 'describeFeatures' beside the reference's module names (`from describeFeatures import *`): not a module of
the reference -- descriptors are an extension -- but scripts that put this directory on PYTHONPATH find
KLTDescribeFeatures and KLTMatchDescriptors here, and through `from selectGoodFeatures import *` as well.  It *is*
pyfeaturetrack_amd.describeFeatures: the name is aliased, not copied.
"""
import sys

import pyfeaturetrack_amd.describeFeatures as _m

sys.modules[__name__] = _m
