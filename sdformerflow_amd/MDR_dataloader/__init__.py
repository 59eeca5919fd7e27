"""The reference's MDR_dataloader (MVSEC / MDR) for the GPU: loader_utils.EventSequence and loader_utils.EventSequenceToVoxelGrid_Pytorch
(the event front end), and loader_utils.DenseSparseAugmentor, whose draws hip.augment_resize_chunk applies on the device.  File readers
are out of scope; the crop, flip and event-drop transforms the DSEC training loops compose are DSEC_dataloader.data_augmentation's."""
