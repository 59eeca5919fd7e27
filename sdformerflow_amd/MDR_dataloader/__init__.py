"""The event front end of the reference's MDR_dataloader (MVSEC / MDR), on the GPU: loader_utils.EventSequence and
loader_utils.EventSequenceToVoxelGrid_Pytorch.  File readers and the MDR augmentor (DenseSparseAugmentor) are out of scope; the crop,
flip and event-drop transforms the training loops compose are DSEC_dataloader.data_augmentation's."""
